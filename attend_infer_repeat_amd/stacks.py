"""Where the stacks of post-parse stages behind AIRonMNIST.parse / parse_tiled / track are specified, built and cached: the normalised
spec of a stack (`stack_spec`), the one builder (`build_stack`), the bounded cache and the single-slot holder of built and captured
stages (`BoundedCache`, `slot`), the keys of the track family (`track_key`, `stitch_spec`, `stream_key`, `stream_smoother_key`, `fit_key`) and the
builder of the stack behind one (`build_track_stack`).  Pure Python; the stage classes are imported where a stack is built.
"""
from collections import namedtuple

StackSpec = namedtuple("StackSpec", "refine lr prune propose temporal")     # int | None, (lr_what, lr_where) | None, the pruner's
#                                                                             candidates | None, (P, rounds) | None, (P, rounds) | None
TrackKey = namedtuple("TrackKey", "S F assoc stack smooth matching device motion motion_gate stitch", defaults=(None, None, None))
#   assoc, smooth, motion: sorted (name, value) pairs; smooth | None, motion | None; motion_gate: the float | None; stitch: None |
#   (max_gap, gate, appearance_weight | None, sorted noise pairs | None) -- `stitch_spec`'s
StreamKey = namedtuple("StreamKey", "S F assoc stack matching device stream")  # a track.StreamTracker's: stream is True (a key of its own)
FitKey = namedtuple("FitKey", "S F assoc stack matching device fit motion motion_gate", defaults=(None, None))      # ... with a trajectory.
#   TrajectoryNoiseFitter: the grids
StreamSmoothKey = namedtuple("StreamSmoothKey", "S F assoc stack matching device stream smooth")      # ... with a trajectory.StreamSmoother


def require_engine(air, who):
    """the training engine of `air`; `who` names the entry that cannot do without it"""
    eng = getattr(air, "_engine", None)
    if eng is None:
        raise NotImplementedError("%s needs the fused engine: call train_step(...) with an engine-eligible "
                                  "configuration first (AIRonMNIST._engine is None on the generic autograd path)" % who)
    return eng


def _per_round(value, text):
    """None | P | (P, rounds) -> None | (P, rounds); a bool is not a count"""
    if value is None:
        return None
    try:
        spec = (int(value), 1) if not isinstance(value, (tuple, list)) else tuple(int(v) for v in value)
    except (TypeError, ValueError):
        spec = ()
    if len(spec) != 2 or isinstance(value, bool):
        raise ValueError(text + ", or (proposals, rounds), got %r" % (value,))
    return spec


def stack_spec(refine=None, refine_lr=None, prune=None, propose=None, temporal=None, who="parse"):
    """The arguments that ask for stages behind a parse, as one hashable StackSpec; `who` names the caller in the refusal."""
    if prune is not None and propose is not None:
        why = ": the search over the candidate pool already contains prune=\"all\"" if who == "parse" else ""
        raise ValueError("%s: prune together with propose is not supported%s; pass one of them" % (who, why))
    lr = None
    if refine is not None:
        from .refine import DEFAULT_LR
        refine, lr = int(refine), tuple(float(v) for v in (DEFAULT_LR if refine_lr is None else refine_lr))
        if len(lr) != 2:
            raise ValueError("refine_lr: (lr_what, lr_where), got %r" % (lr,))
    return StackSpec(refine, lr, prune, _per_round(propose, "propose: the number of proposals per round"),
                     _per_round(temporal, "temporal: the number of neighbour proposals per round"))


def smooth_spec(smooth, stream=False):
    """smooth=None | True | dict(horizon=, process_noise=, measurement_noise=, velocity_var=) -> None | the full dict; stream=True
    (`stream_smooth_spec`): a dict may carry lag= too (None: max_age), and there is no None: the caller asked for a smoother"""
    from .trajectory import DEFAULTS
    if not stream and (smooth is None or smooth is False):
        return None
    spec = dict(DEFAULTS, lag=None, horizon=0) if stream else dict(DEFAULTS, horizon=0)
    if smooth is not True:
        if not isinstance(smooth, dict) or set(smooth) - set(spec):
            raise ValueError("smooth: %s or a dict with keys among %s, got %r" % ("True" if stream else "None, True", sorted(spec), smooth))
        spec.update(smooth)
    try:
        spec["process_noise"] = tuple(float(v) for v in spec["process_noise"])
    except TypeError:
        raise ValueError("smooth: process_noise must be two numbers (q_shift, q_scale), got %r" % (spec["process_noise"],))
    return spec


STITCH_KEYS = ("max_gap", "gate", "appearance_weight", "process_noise", "measurement_noise", "velocity_var")


def stitch_spec(stitch):
    """stitch=None | False (off), True (the defaults), MAX_GAP (an integer) or a dict with any of STITCH_KEYS -> None | (max_gap, gate,
    appearance_weight | None, sorted noise pairs | None), checked by track.check_stitch: appearance_weight None is the tracker's, noise
    None the tracker's motion terms or trajectory.DEFAULTS (track.TrackStitcher's rule); noise terms given are completed by the defaults"""
    from . import track as tr
    if stitch is None or stitch is False:
        return None
    spec = {}
    if isinstance(stitch, dict):
        unknown = sorted(set(stitch) - set(STITCH_KEYS), key=str)
        if unknown:
            raise ValueError("stitch: unknown keys %r; it takes %s" % (unknown, ", ".join(STITCH_KEYS)))
        spec = {k: v for k, v in stitch.items() if v is not None}
    elif stitch is not True:
        spec = dict(max_gap=stitch)
    noise = {k: spec[k] for k in STITCH_KEYS[3:] if k in spec}
    w = spec.get("appearance_weight")
    max_gap, gate, _, terms = tr.check_stitch(spec.get("max_gap", tr.STITCH_MAX_GAP), spec.get("gate", True),
                                              tr.DEFAULTS["appearance_weight"] if w is None else w, noise or None)
    return (max_gap, gate, None if w is None else float(w), tuple(sorted(terms.items())) if noise else None)


def track_key(eng, n_sequences, n_frames, iou_gate=None, appearance_weight=None, birth_score=None, max_age=None, refine=None,
              refine_lr=None, prune=None, propose=None, temporal=None, smooth=None, matching=None, motion=None, motion_gate=None,
              stitch=None):
    """The arguments of the track family, normalised once and checked against the engine `eng` (track, temporal and trajectory
    check_arguments, before anything is built): None for an association argument is track.DEFAULTS, temporal=None, smooth=None,
    matching=None | "greedy" and motion=None give the very key of a call without the argument.  motion=True together with
    smooth=dict(...) takes the smoother's noise terms; an explicit motion=dict(...) wins.  motion_gate=None | False is the key of a call
    without it, True is track.MOTION_GATE_DEFAULT, and a gate without motion is refused (track.check_motion_gate).  stitch=None | False
    is the key of a call without it; True | MAX_GAP | dict(...) (`stitch_spec`) asks for a track.TrackStitcher behind the tracker -- with
    smooth= it is refused (track.STITCH_WITH_SMOOTH), with temporal=, a provider, it is not."""
    from . import track as tr
    stack = stack_spec(refine, refine_lr, prune, propose, temporal, who="track")
    stitch = stitch_spec(stitch)
    if stitch is not None and smooth_spec(smooth) is not None:
        raise ValueError(tr.STITCH_WITH_SMOOTH)
    given = dict(iou_gate=iou_gate, appearance_weight=appearance_weight, birth_score=birth_score, max_age=max_age)
    assoc = {k: (tr.DEFAULTS[k] if v is None else v) for k, v in given.items()}
    S, F = int(n_sequences), int(n_frames)
    matching = "greedy" if matching is None else matching
    tr.check_arguments(eng.cfg.max_steps, F, S * F if S >= 1 else None, matching=matching, **assoc)
    if S < 1:
        raise ValueError("track: at least one sequence, got %r" % (n_sequences,))
    if stack.temporal is not None:
        from .temporal import check_arguments as check_temporal
        check_temporal(eng.cfg, F, S * F, *stack.temporal)
    smooth = smooth_spec(smooth)
    if smooth is not None:
        from .trajectory import check_arguments as check_smooth
        check_smooth(eng.cfg.max_steps, F, S * F, assoc["max_age"], **smooth)
        if motion is True:
            motion = {k: smooth[k] for k in ("process_noise", "measurement_noise", "velocity_var")}
        smooth = tuple(sorted(smooth.items()))
    motion = tr.check_motion(motion)
    motion_gate = tr.check_motion_gate(motion_gate, motion)
    if motion is not None:
        motion = tuple(sorted(motion.items()))
    assoc = {k: (int(v) if k == "max_age" else float(v)) for k, v in assoc.items()}
    return TrackKey(S, F, tuple(sorted(assoc.items())), stack, smooth, matching, str(eng.device), motion, motion_gate, stitch)


def stream_key(eng, n_sequences, chunk_frames, motion=None, motion_gate=None, **track_args):
    """The arguments of a stream tracker, normalised and checked as `track_key` does (`track_args` are its arguments; there is no
    smooth= among a stream tracker's): a key of its own in the cache of the track family, never that of a one-shot tracker with the
    same arguments.  motion and motion_gate: refused (out of scope on a stream)."""
    if (motion is not None and motion is not False) or (motion_gate is not None and motion_gate is not False):
        from .track import MOTION_ON_A_STREAM
        raise ValueError(MOTION_ON_A_STREAM)
    for name in ("smooth", "stitch"):
        if name in track_args:
            raise TypeError("stream_key() got an unexpected keyword argument %r" % name)
    k = track_key(eng, n_sequences, chunk_frames, **track_args)
    return StreamKey(k.S, k.F, k.assoc, k.stack, k.matching, k.device, True)


def stream_smooth_spec(smooth):
    """smooth=True | dict(lag=, horizon=, process_noise=, measurement_noise=, velocity_var=) -> the full dict (lag None: max_age)"""
    return smooth_spec(smooth, stream=True)


def stream_smoother_key(eng, n_sequences, chunk_frames, smooth=True, **stream_args):
    """The key of a stream tracker with a trajectory.StreamSmoother behind it, checked by trajectory.check_stream_arguments before
    anything is built: `stream_key`'s fields and the smoother's arguments -- a key of its own, never that of the stream tracker with
    the same arguments (the two are different streams)."""
    from .trajectory import check_stream_arguments
    k = stream_key(eng, n_sequences, chunk_frames, **stream_args)
    spec = stream_smooth_spec(smooth)
    L = check_stream_arguments(eng.cfg.max_steps, k.F, k.S * k.F, dict(k.assoc)["max_age"], **spec)[4]
    return StreamSmoothKey(k.S, k.F, k.assoc, k.stack, k.matching, k.device, True, tuple(sorted(dict(spec, lag=L).items())))


def fit_key(eng, n_sequences, n_frames, shift_ratios=None, scale_ratios=None, velocity_ratio=None, **track_args):
    """The key of a tracker with a trajectory.TrajectoryNoiseFitter behind it, checked by trajectory.check_fit_arguments before
    anything is built: `track_key`'s fields (without a smoother) and the fitter's grids -- a key of its own."""
    from .trajectory import check_fit_arguments
    if track_args.get("smooth") is not None:
        raise ValueError("fit_track_noise: the noise terms are fitted to the tracker's sightings; smooth= has no part in it")
    if track_args.get("stitch") not in (None, False):
        raise ValueError("fit_track_noise: the noise terms are fitted to the tracker's sightings; stitch= has no part in it")
    k = track_key(eng, n_sequences, n_frames, **dict(track_args, smooth=None, stitch=None))
    fit = check_fit_arguments(eng.cfg.max_steps, k.F, k.S * k.F, shift_ratios, scale_ratios, velocity_ratio)[3:]
    return FitKey(k.S, k.F, k.assoc, k.stack, k.matching, k.device, fit, k.motion, k.motion_gate)


def stage_classes():
    from .propose import ParseProposer
    from .prune import ParsePruner
    from .refine import ParseRefiner
    from .temporal import TemporalProposer
    return ParseRefiner, ParsePruner, ParseProposer, TemporalProposer


def build_stack(base, spec, n_frames=None, classes=None):
    """[base, refiner?, pruner?, proposer?, temporal proposer?]: the stages `spec` asks for, each bound to the one before it (the
    temporal proposer over sequences of `n_frames` frames).  classes: the four constructors in that order (None: stage_classes())."""
    ParseRefiner, ParsePruner, ParseProposer, TemporalProposer = stage_classes() if classes is None else classes
    stack = [base]
    if spec.refine is not None:
        stack.append(ParseRefiner(stack[-1], spec.refine, spec.lr[0], spec.lr[1]))
    if spec.prune is not None:
        stack.append(ParsePruner(stack[-1], spec.prune))
    if spec.propose is not None:
        stack.append(ParseProposer(stack[-1], spec.propose[0], spec.propose[1]))
    if spec.temporal is not None:
        stack.append(TemporalProposer(stack[-1], n_frames, spec.temporal[0], spec.temporal[1]))
    return stack


def track_classes():
    from .track import SequenceTracker, StreamTracker
    from .trajectory import StreamSmoother, TrajectoryNoiseFitter, TrajectorySmoother
    return SequenceTracker, StreamTracker, TrajectorySmoother, StreamSmoother, TrajectoryNoiseFitter


def build_track_stack(stack, key, classes=None, stitcher=None):
    """`stack` (a provider stack, `build_stack`'s) with what a key of the track family asks for behind it: a SequenceTracker (TrackKey,
    FitKey: with the key's motion and gate) or a StreamTracker (StreamKey, StreamSmoothKey) bound to its last member, then -- bound to
    that tracker -- a TrajectorySmoother (TrackKey with smooth), a StreamSmoother (StreamSmoothKey), a TrajectoryNoiseFitter (FitKey)
    or nothing; a TrackKey with stitch: a track.TrackStitcher bound to the tracker (never with smooth: `track_key` refuses that).
    classes: the five constructors in that order (None: track_classes()); stitcher: TrackStitcher's (None: the class)."""
    SequenceTracker, StreamTracker, Smoother, StreamSmoother, Fitter = track_classes() if classes is None else classes
    on_stream = isinstance(key, (StreamKey, StreamSmoothKey))
    rule = dict(key.assoc, matching=key.matching)
    if on_stream:
        stack.append(StreamTracker(stack[-1], key.F, **rule))
    else:
        stack.append(SequenceTracker(stack[-1], key.F, motion=key.motion and dict(key.motion), motion_gate=key.motion_gate, **rule))
    if isinstance(key, FitKey):
        stack.append(Fitter(stack[-1], *key.fit))
    elif getattr(key, "smooth", None) is not None:
        stack.append((StreamSmoother if on_stream else Smoother)(stack[-1], **dict(key.smooth)))
    elif getattr(key, "stitch", None) is not None:
        if stitcher is None:
            from .track import TrackStitcher as stitcher
        max_gap, gate, w, noise = key.stitch
        stack.append(stitcher(stack[-1], max_gap=max_gap, gate=gate, appearance_weight=w, noise=noise and dict(noise)))
    return stack


def _members(entry):
    return entry if isinstance(entry, list) else [entry]


def captured(entry):
    """`entry` (a stage, or a stack) with every member captured, in stack order"""
    for s in _members(entry):
        s.capture()
    return entry


def release(entry):
    """release the graphs of `entry` (a stage, or a stack: every member, last stage first)"""
    for s in reversed(_members(entry)):
        s.release_graphs()


class BoundedCache(dict):
    """key -> a built and captured stage or stack, least recently used first; at most limit() entries (the limit is read when used)"""

    def __init__(self, limit):
        super().__init__()
        self.limit = limit

    def get(self, key, build, valid=None):
        """the entry under `key`, now the most recently used: build() on a miss -- a hit that valid() refuses is released and counts as
        one -- then the oldest entries are released while there are more than the limit"""
        entry = self.pop(key, None)
        if entry is not None and valid is not None and not valid(entry):
            release(entry)
            entry = None
        if entry is None:
            entry = build()
        self[key] = entry
        while len(self) > self.limit():
            release(self.pop(next(iter(self))))
        return entry

    def drop(self, predicate):
        """release and forget every entry that predicate(entry) names"""
        for key in [k for k, e in self.items() if predicate(e)]:
            release(self.pop(key))


def slot(owner, name, current, build):
    """The single-slot holder: `owner.<name>` when there is one and current(it) holds; else what build() makes, captured, the old one
    released."""
    s = getattr(owner, name, None)
    if s is None or not current(s):
        if s is not None:
            s.release_graphs()
        s = build()
        s.capture()
        setattr(owner, name, s)
    return s
