"""Read-out of an engine's launch plans as text (plumbing, like `AIREngine.outputs()`): one line per plan entry with its position, the
C symbol, the entry name and every argument, so that two builds of the plans -- before and after a change of the builder, or two
`_build_plans()` calls on one engine -- can be compared byte for byte.

Scalars are written by `repr`, ctypes scalars by value, `byref(x)` and struct arrays field by field.  Every device pointer (a
`c_void_p` argument or struct field) is written as `<name>+<byte offset>`, where <name> is the engine tensor whose storage holds the
address: the map is built by walking the engine's attributes, dicts, lists and `_Mlp` objects (the workspace, the bf16 mirrors, the
observation ring and the feeder's dataset included).  A pointer that resolves to nothing is an error, never a raw address.

Reads only attributes every engine with `_build_plans` has; imports nothing of the package but the ctypes mirrors."""
import ctypes

PLANS = ("_plan_rng", "_plan_fwd", "_plan_fwd_noise", "_plan_fwd_train", "_plan_bwd", "_plan_opt", "_plan_bwd_riders", "_plan_opt_rest")
FLAGS = ("_rng_inc", "_defer_dw", "_use16", "_fold_gx", "_what_head", "_fold_gauss_bwd")
_SKIP = ("_keep", "_rider_slices_all") + PLANS            # ctypes objects and the plans themselves: nothing to name there


def _is_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "untyped_storage")


def _walk(obj, path, out, depth=0):
    if _is_tensor(obj):
        if obj.is_cuda:
            out.append((path, obj))
    elif isinstance(obj, dict):
        for i, (k, v) in enumerate(obj.items()):
            _walk(v, "%s[%s]" % (path, k) if isinstance(k, str) else "%s{%d}" % (path, i), out, depth + 1)   # (non-string keys are addresses)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _walk(v, "%s[%d]" % (path, i), out, depth + 1)
    elif type(obj).__name__ == "_Mlp" and depth < 2:
        for k, v in sorted(vars(obj).items()):
            _walk(v, "%s.%s" % (path, k), out, depth + 1)


def pointer_map(engine):
    """[(lo, hi, name)] of every device storage an engine attribute reaches, sorted; the name of a storage is that of the tensor that
    starts lowest in it (then the largest, then the first by name)"""
    found = []
    for k, v in sorted(vars(engine).items()):
        if k not in _SKIP:
            _walk(v, k, found)
    best = {}
    for name, t in found:
        st = t.untyped_storage()
        lo = st.data_ptr()
        key = (t.data_ptr() - lo, -t.numel() * t.element_size(), name)
        if lo not in best or key < best[lo][0]:
            best[lo] = (key, lo + st.nbytes(), name)
    return sorted((lo, hi, name) for lo, (_, hi, name) in best.items())


class _Writer:
    def __init__(self, engine):
        self.spans = pointer_map(engine)

    def ptr(self, value):
        if not value:
            return "NULL"
        value = int(value)
        for lo, hi, name in self.spans:
            if lo <= value < hi:
                return "%s+%d" % (name, value - lo)
        raise LookupError("plan pointer 0x%x lies in no tensor the engine holds" % value)

    def field(self, ctype, value):
        if ctype is ctypes.c_void_p:
            return self.ptr(value)
        if isinstance(value, ctypes.Array):
            return "[" + ", ".join(self.field(value._type_, v) for v in value) + "]"
        if isinstance(value, ctypes.Structure):
            return self.struct(value)
        return repr(value)

    def struct(self, s):
        return "{" + ", ".join("%s=%s" % (n, self.field(t, getattr(s, n))) for n, t in s._fields_) + "}"

    def arg(self, a):
        if a is None:
            return "None"
        if isinstance(a, ctypes.c_void_p):
            return self.ptr(a.value)
        if isinstance(a, ctypes._SimpleCData):
            return repr(a.value)
        if isinstance(a, ctypes.Structure):
            return self.struct(a)
        if isinstance(a, ctypes.Array):
            return self.field(a._type_, a)
        if hasattr(a, "_obj"):                               # ctypes.byref(x)
            return "&" + self.arg(a._obj)
        if isinstance(a, (bool, int, float, str)):
            return repr(a)
        raise TypeError("plan argument of type %s" % type(a).__name__)

    def plan(self, title, plan, out):
        if plan is None:
            out.append("== %s: None" % title)
            return
        out.append("== %s: %d entries" % (title, len(plan)))
        for i, (fn, args, name) in enumerate(plan):
            # (an address passed as a plain int -- a descriptor field handed on -- is known by the C signature)
            types = list(getattr(fn, "argtypes", None) or []) + [None] * len(args)
            out.append("%3d %s %s (%s)" % (i, fn.__name__, name, ", ".join(
                self.ptr(a) if t is ctypes.c_void_p and isinstance(a, int) else self.arg(a) for a, t in zip(args, types))))


def describe_plans(engine) -> str:
    """every plan and list the rest of the package reads off a built engine, as text (see the module docstring)"""
    w, out = _Writer(engine), []
    for name in PLANS:
        w.plan(name, getattr(engine, name), out)
    w.plan("_opt_calls_factory(0.5)", engine._opt_calls_factory(0.5), out)
    out.append("== _grad_buckets: %r" % (list(engine._grad_buckets),))
    out.append("== tail_bucket(): %r" % (engine.tail_bucket(),))
    out.append("== kernel_launch_count(): %r" % (sorted(engine.kernel_launch_count().items()),))
    out.append("== flags: " + ", ".join("%s=%r" % (k, getattr(engine, k)) for k in FLAGS))
    out.append("== _kl_weights: " + w.ptr(engine._kl_weights.data_ptr()))
    # (the attributes below are published by the phase that decides them, and only then)
    if getattr(engine, "_feeder", None) is not None:
        out.append("== _fold_gather: %r" % (engine._fold_gather,))
    if engine._use16:
        out.append("== _dx_chain_launches: %r" % (engine._dx_chain_launches,))
    if engine._plan_bwd_riders is not None:
        out.append("== _rider_slices: " + " ".join(w.struct(s) for s in engine._rider_slices))
        out.append("== _fold: " + ("None" if engine._fold is None else w.struct(engine._fold)))
        if engine._fold is not None:
            out.append("== _fold_early: " + ("None" if engine._fold_early is None else w.struct(engine._fold_early)))
    return "\n".join(out) + "\n"
