"""Developer probe: the launch plans of an engine as text (run on the GPU box); a front end of
attend_infer_repeat_amd/plan_describe.py.

   python tools/probes/plan_dump.py [c2|c4|c5] [batch]         the train step's launch list with the problems of every grouped GEMM
   python tools/probes/plan_dump.py --describe [c2|c4|c5] [batch]   every plan, every argument, pointers by tensor name
   python tools/probes/plan_dump.py --matrix DIR               one --describe file per variant of a fixed matrix (regimes, shapes,
                                                               switches, rebuilds) + DIR/SHA256SUMS: the builder's regression record

The matrix builds a fresh engine per variant in one process with the variant's environment; it launches nothing beyond what
construction launches.  A variant that raises records the error instead."""
import ast, hashlib, os, sys
import torch
from attend_infer_repeat_amd.engine import AIREngine, EngineConfig
from attend_infer_repeat_amd.plan_describe import describe_plans

C4 = dict(img_size=(100, 100), crop_size=(28, 28), max_steps=5)
BF = dict(mfma_dtype="bf16")


def summary(eng):
    lines, i = [], 0
    for plan in eng._single_gpu_step_plans():
        for fn, args, name in plan:
            line = "%2d %-34s" % (i, name)
            if name in ("air_gemm", "air_gemm_bf16"):
                line += "ta=%d tb=%d %dx%dx%d epi=%s" % (args[0], args[1], args[2], args[3], args[4], args[12])
            if name.startswith("air_gemm_grouped"):
                arr, n = args[0], args[1]
                probs = []
                for j in range(n):
                    d = arr[j]
                    t16 = ((d.M + 15) // 16) * ((d.N + 15) // 16)
                    probs.append("%s%s %dx%dx%d(%d)%s" % ("T" if d.ta else "N", "T" if d.tb else "N", d.M, d.N, d.K, t16, "+cs" if d.colsum else ""))
                line += " | ".join(probs)
            lines.append(line)
            i += 1
    return "\n".join(lines)


def test_switches():
    """SWITCHES of tests/test_engine.py, read from its source (the module itself needs the oracle and a device)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests", "test_engine.py")
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "SWITCHES":
            return eval(compile(ast.Expression(node.value), path, "eval"), {"dict": dict})
    raise LookupError("SWITCHES not found in tests/test_engine.py")


def attach(shuffle):
    def post(eng):
        P = eng.obs.shape[1]
        eng.attach_dataset(torch.zeros(300, P, device=eng.device), shuffle=shuffle, seed=5)
    return post


def knob(**changes):
    return lambda eng: eng.update_config(**changes)


def world2(eng):
    eng.world_size = 2
    eng._build_plans()


def matrix():
    """[(name, cfg kwargs, batch, environment, action on the built engine or None)]"""
    v = [("default_b%d" % b, {}, b, {}, None) for b in (1, 8, 50, 64, 272, 704, 1024)]
    v += [("c4_b%d" % b, C4, b, {}, None) for b in (8, 64)]
    v += [("bf16_b64", BF, 64, {}, None), ("bf16_b1024", BF, 1024, {}, None), ("bf16_b64_t12", dict(BF, max_steps=12), 64, {}, None)]
    for name, kw in test_switches().items():
        v += [("switch_%s_b%d" % (name, b), kw, b, {}, None) for b in (8, 64)]
    v += [("arch_enc1", dict(inpt_encoder_hidden=(256,)), 64, {}, None),
          ("arch_ge1", dict(glimpse_encoder_hidden=(256,)), 64, {}, None),
          ("arch_bl4", dict(baseline_hidden=(256, 128, 64, 32)), 64, {}, None),
          ("arch_pix_odd", dict(img_size=(49, 51)), 64, {}, None)]
    for key in ("AIR_SPLIT_K0=0", "AIR_FOLD_GX=0", "AIR_FUSE_WHAT_HEAD=0", "AIR_FUSE_GAUSS_BWD=0", "AIR_LSTM_BWD_ENTRY=0", "AIR_LSTM_DW_EARLY=0",
                "AIR_OPT_RIDERS=0", "AIR_OPT_FOLD=0", "AIR_FUSE_CANVAS=0", "AIR_CANVAS_SPLIT=1", "AIR_FUSE_ATTEND_M=0"):
        v.append(("env_%s_b64" % key, {}, 64, dict([key.split("=")]), None))
    v.append(("env_AIR_FUSE_CANVAS=1_c4_b64", C4, 64, {"AIR_FUSE_CANVAS": "1"}, None))
    for key in ("AIR_FUSE_LSTM_WIDE=0", "AIR_DEFER_DW_MIN_ROWS=100000000", "AIR_FUSE_CANVAS_THROUGHPUT=1"):
        v.append(("env_%s_b1024" % key, {}, 1024, dict([key.split("=")]), None))
    for key in ("AIR_BF16_STORAGE=0", "AIR_BF16_LSTM=0", "AIR_FUSE_PROLOGUE_CVT=0", "AIR_DX_CHAIN=1"):
        v.append(("env_%s_bf16_b1024" % key, BF, 1024, dict([key.split("=")]), None))
    for tag, kw, b in (("b64", {}, 64), ("bf16_b1024", BF, 1024)):
        for shuffle in (True, False):
            for env in ({}, {"AIR_FOLD_GATHER": "0"}):
                v.append(("dataset_%s_shuffle%d%s" % (tag, shuffle, "_nofold" if env else ""), kw, b, env, attach(shuffle)))
    v += [("rebuild_use_prior_off_b64", {}, 64, {}, knob(use_prior=False)),
          ("rebuild_output_multiplier_b64", {}, 64, {}, knob(output_multiplier=0.5)),
          ("rebuild_after_capture3_b64", {}, 64, {}, lambda eng: eng.capture(steps_per_replay=3)),
          ("rebuild_world2_b64", {}, 64, {}, world2)]
    return v


def run_matrix(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    base, sums = dict(os.environ), []
    for name, kw, B, env, post in matrix():
        os.environ.clear(); os.environ.update(base); os.environ.update(env)
        try:
            eng = AIREngine(EngineConfig(**kw), B, device=torch.device("cuda", 0), seed=1)
            if post is not None:
                post(eng)
            text = describe_plans(eng)
            eng.release_graphs()
            del eng
        except Exception as e:                                   # recorded: both sides of a comparison must raise the same
            text = "raised %s: %s\n" % (type(e).__name__, e)
        with open(os.path.join(out_dir, name + ".txt"), "w") as f:
            f.write(text)
        sums.append("%s  %s.txt" % (hashlib.sha256(text.encode()).hexdigest(), name))
        print(sums[-1], flush=True)
    os.environ.clear(); os.environ.update(base)
    with open(os.path.join(out_dir, "SHA256SUMS"), "w") as f:
        f.write("\n".join(sums) + "\n")
    print("%d variants" % len(sums))


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--matrix"]:
        run_matrix(argv[1])
        sys.exit(0)
    describe = argv[:1] == ["--describe"]
    argv = argv[1:] if describe else argv
    cfgname = argv[0] if argv else "c2"
    kw, B = (C4 if cfgname == "c4" else {}), (int(argv[1]) if len(argv) > 1 else 64)
    if cfgname == "c5":
        kw, B = BF, (int(argv[1]) if len(argv) > 1 else 1024)
    eng = AIREngine(EngineConfig(**kw), B, device=torch.device("cuda", 0), seed=1, keep_canvas_steps=True)
    print(describe_plans(eng) if describe else summary(eng), end="" if describe else "\n")
