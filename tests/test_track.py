"""GPU tests of sequence tracking (attend_infer_repeat_amd/track.py, csrc/track_kernels.hip): air_track_associate against
track.reference_associate on crafted fp32 rows (margins asserted), air_track_owner against numpy bit for bit, air_track_score against
track.reference_score, then SequenceTracker: the composition provider.parse() -> association against the host reference, the provider's
result untouched, graph replay against eager, permuted sequences, one frame, a second provider, the totals and the model's surface.

Bars.  Everything the association decides is compared exactly, on inputs whose decisions are not within rounding of flipping: every
IoU at least MARGIN from the gate, every greedy round's winner at least MARGIN ahead of the runner-up (except the planted ties, where the
rule's tie order decides).  The float64 formulas are differences, products, sums and divisions of numbers of order 1e-3 .. 1e3, evaluated
operation by operation in the same order on both sides, so two evaluations differ by less than 1e-13; `affinity` is that float64 rounded
once to fp32 and is compared by bits.  seq_iou is a sum of at most F * G float64 IoUs in one stated order: 1e-12 relative."""
import json
import os

import numpy as np
import pytest
import torch

from test_parse import SENTINEL_F, SENTINEL_I, _mnist_air, _train_state, e2e_case, make_parser
from test_track_host import OUTPUTS, TIE_ONE_TRACK, TIE_TWO_TRACKS, _overflow_frames, build_rows, crafted_rows, moving_gt

from attend_infer_repeat_amd import track

pytestmark = pytest.mark.gpu

MARGIN, TAIL = 1e-9, 64
dev_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
DTYPES = dict(track_id=torch.int32, obj_state=torch.int8, affinity=torch.float32, prev_frame=torch.int32, prev_slot=torch.int32,
              num_tracks=torch.int32, track_first=torch.int32, track_last=torch.int32, track_length=torch.int32, track_gaps=torch.int32,
              state_counts=torch.int32)


def sentinel(shape, dtype, tail=TAIL):
    """a flat sentinel-filled buffer of prod(shape) + tail elements"""
    fill = SENTINEL_F if dtype.is_floating_point else (99 if dtype in (torch.int8, torch.int16) else SENTINEL_I)
    return torch.full((int(np.prod(shape)) + tail,), fill, dtype=dtype, device="cuda"), fill


# ---- 1. air_track_associate -----------------------------------------------------------------------------------------------------------
def run_associate(case, **kw):
    """air_track_associate alone (current stream); every output and a tail behind it start as a sentinel fill"""
    from attend_infer_repeat_amd import hip as Hh
    T, A, S, F = case["T"], case["A"], case["S"], case["F"]
    R = S * F
    shapes = dict(track_id=(T, R), obj_state=(T, R), affinity=(T, R), prev_frame=(T, R), prev_slot=(T, R), num_tracks=(S,),
                  track_first=(S, F * T), track_last=(S, F * T), track_length=(S, F * T), track_gaps=(S, F * T), state_counts=(S, 6))
    bufs = {k: sentinel(shapes[k], DTYPES[k]) for k in OUTPUTS}
    d = {k: dev_t(case[k]) for k in ("what", "boxes", "score")}
    d["n"] = dev_t(case["n"].astype(np.int32))
    p = Hh._p
    assoc = dict(track.DEFAULTS)
    assoc.update(case.get("kw", {}))
    a = dict(what=p(d["what"]), boxes=p(d["boxes"]), score=p(d["score"]), n=p(d["n"]), T=T, S=S, F=F, R=R, A=A, **assoc)
    a.update({k: p(bufs[k][0]) for k in OUTPUTS})
    a.update(kw)
    st = Hh.lib().air_track_associate(a["what"], a["boxes"], a["score"], a["n"], a["T"], a["S"], a["F"], a["R"], a["A"], float(a["iou_gate"]),
                                      float(a["appearance_weight"]), float(a["birth_score"]), int(a["max_age"]),
                                      *[a[k] for k in OUTPUTS], Hh._stream())
    torch.cuda.synchronize()
    got, tails = {}, {}
    for k in OUTPUTS:
        n = int(np.prod(shapes[k]))
        got[k], tails[k] = bufs[k][0][:n].view(shapes[k]).cpu().numpy(), bool((bufs[k][0][n:] == bufs[k][1]).all())
    return st, got, tails, {k: bufs[k][1] for k in OUTPUTS}


def check_associate(got, ref, tails):
    for k in OUTPUTS:
        assert tails[k], k
        if k == "affinity":
            assert np.array_equal(bits(got[k]), bits(ref[k])), k
        else:
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])


ASSOC_PARAMS = [(1, 1, 1, 1), (1, 5, 3, 5), (3, 1, 1, 2), (3, 5, 3, 5), (3, 50, 1, 17), (6, 5, 3, 2), (6, 50, 3, 5), (6, 1, 1, 17),
                (32, 5, 1, 5), (32, 50, 3, 2), (32, 1, 3, 1), (3, 50, 3, 17), (6, 5, 1, 1)]


@pytest.mark.parametrize("T,A,S,F", ASSOC_PARAMS)
def test_associate_is_the_reference(gpu_device, T, A, S, F):
    kw = dict(iou_gate=0.2, appearance_weight=0.6, birth_score=0.4, max_age=2) if (T + A + S + F) % 2 else {}
    case, ref = crafted_rows(T, A, S, F, seed=T + A + S + F, margin=MARGIN, **kw)
    assert (ref["gate_margin"] >= MARGIN).all() and (ref["round_margin"] >= MARGIN).all()
    st, got, tails, _ = run_associate(case)
    assert st == 0
    check_associate(got, ref, tails)
    print("states", ref["state_counts"].sum(0).tolist(), "tracks", ref["num_tracks"].tolist())
    assert (got["state_counts"].sum(1) == T * F).all()


def test_associate_planted_ties_overflow_and_nothing_present(gpu_device):
    for frames, T in ((TIE_ONE_TRACK, 2), (TIE_TWO_TRACKS, 2), ([TIE_TWO_TRACKS[0][::-1], TIE_TWO_TRACKS[1]], 2)):
        what, boxes, score, n = build_rows(frames, T)
        case = dict(what=what, boxes=boxes, score=score, n=n, T=T, A=2, S=1, F=2)
        ref = track.reference_associate(what, boxes, score, n, 2, return_margins=True)
        assert ref["round_margin"][0] == 0.0                       # an exact tie: the rule's order decides
        st, got, tails, _ = run_associate(case)
        assert st == 0
        check_associate(got, ref, tails)
    for F, max_age in ((4, 1), (3, 0)):                            # 32 coasting tracks hold every slot
        what, boxes, score, n = build_rows(_overflow_frames(F), 32, 3)
        case = dict(what=what, boxes=boxes, score=score, n=n, T=32, A=3, S=1, F=F, kw=dict(max_age=max_age))
        ref = track.reference_associate(what, boxes, score, n, F, max_age=max_age)
        st, got, tails, _ = run_associate(case)
        assert st == 0 and got["state_counts"][0, track.OVERFLOW] == 32 * (F - 2) and got["num_tracks"][0] == 64
        check_associate(got, ref, tails)
    case, _ = crafted_rows(3, 5, 3, 5, seed=2)
    case["n"][:] = 0
    st, got, tails, _ = run_associate(case)
    assert st == 0 and all(tails.values()) and (got["track_id"] == -1).all() and (got["obj_state"] == 0).all()
    assert (got["num_tracks"] == 0).all() and (got["track_first"] == -1).all() and (got["track_length"] == 0).all()
    assert got["state_counts"].tolist() == [[15, 0, 0, 0, 0, 0]] * 3 and (got["affinity"] == 0).all() and (got["prev_slot"] == -1).all()


def test_associate_argument_checks_write_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case, _ = crafted_rows(3, 5, 2, 4, seed=8)
    off = torch.zeros(3 * 8 * 4 + 1, device="cuda")
    big = dict(what=np.zeros((32, 1, 1), np.float32), boxes=np.zeros((32, 1, 4), np.float32), score=np.zeros((32, 1), np.float32),
               n=np.zeros(1, np.int32), T=32, A=1, S=1, F=1)
    nan = float("nan")
    for kw, code in ((dict(what=None), -1), (dict(boxes=None), -1), (dict(n=None), -1), (dict(track_id=None), -1),
                     (dict(obj_state=None), -1), (dict(state_counts=None), -1), (dict(T=0), -2), (dict(T=33), -2), (dict(S=0), -2),
                     (dict(F=0), -2), (dict(A=0), -2), (dict(R=9), -2), (dict(R=7), -2), (dict(S=4, F=2, R=6), -2),
                     (dict(iou_gate=1.0), -2), (dict(iou_gate=-0.5), -2), (dict(iou_gate=nan), -2), (dict(appearance_weight=1.01), -2),
                     (dict(appearance_weight=-0.1), -2), (dict(appearance_weight=nan), -2), (dict(birth_score=1.5), -2),
                     (dict(birth_score=nan), -2), (dict(max_age=-1), -2), (dict(boxes=Hh._p(off[1:])), -3)):
        st, got, tails, fill = run_associate(case, **kw)
        assert st == code, kw
        assert all(tails.values()) and all((got[k] == fill[k]).all() for k in OUTPUTS), kw
    st, got, tails, fill = run_associate(big, F=1024, S=1, R=1024)  # 1024 * 32 ids do not fit int16 (nothing is read: refused first)
    assert st == -2 and all((got[k] == fill[k]).all() for k in OUTPUTS)


# ---- 2. air_track_owner ---------------------------------------------------------------------------------------------------------------
def run_owner(owner_dev, ids_dev, n_steps, out_offset=0, **kw):
    """air_track_owner alone; owner_dev: an int8 device tensor [R, H, W] (possibly a view at an odd offset), ids_dev [T, R]"""
    from attend_infer_repeat_amd import hip as Hh
    R, H, W = owner_dev.shape
    flat, fill = sentinel((R, H, W), torch.int16, tail=TAIL + out_offset)
    out = flat[out_offset:]
    a = dict(owner=Hh._p(owner_dev), ids=Hh._p(ids_dev), T=n_steps, R=R, H=H, W=W, out=Hh._p(out))
    a.update(kw)
    st = Hh.lib().air_track_owner(a["owner"], a["ids"], a["T"], a["R"], a["H"], a["W"], a["out"], Hh._stream())
    torch.cuda.synchronize()
    n = R * H * W
    return st, out[:n].view(R, H, W).cpu().numpy(), bool((out[n:] == fill).all() and (flat[:out_offset] == fill).all())


def owner_reference(owner, ids, T):
    lut = np.concatenate([ids.astype(np.int16), np.full((1, ids.shape[1]), -1, np.int16)])       # row T: everything outside 0..T-1
    idx = np.where((owner >= 0) & (owner < T), owner, T).astype(np.int64)
    return lut[idx, np.arange(owner.shape[0])[:, None, None]]


@pytest.mark.parametrize("name,R,H,W,T,in_off,out_off", [("word_5x7", 3, 5, 7, 3, 0, 0), ("vector_8x16", 4, 8, 16, 6, 0, 0),
                                                         ("unaligned_in", 3, 8, 16, 3, 3, 0), ("out_on_8", 3, 8, 16, 3, 0, 4),
                                                         ("out_on_2", 3, 8, 16, 3, 0, 1), ("both_off", 5, 9, 13, 32, 5, 3),
                                                         ("50x50", 6, 50, 50, 3, 0, 0), ("many_rows", 5000, 3, 5, 2, 1, 0)])
def test_owner_is_numpy_bit_for_bit(gpu_device, name, R, H, W, T, in_off, out_off):
    rng = np.random.default_rng(sum(map(ord, name)))
    owner = rng.integers(-1, T, (R, H, W)).astype(np.int8)
    owner.reshape(-1)[rng.integers(0, owner.size, max(owner.size // 20, 2))] = rng.choice([T, 100, -2, -128, 127])      # outside -1 .. T-1
    ids = rng.integers(-1, 32767, (T, R)).astype(np.int32)
    flat = torch.zeros(owner.size + in_off, dtype=torch.int8, device="cuda")
    flat[in_off:] = dev_t(owner).reshape(-1)
    st, got, clean = run_owner(flat[in_off:].view(R, H, W), dev_t(ids), T, out_off)
    assert st == 0 and clean
    want = owner_reference(owner, ids, T)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert (want[(owner < 0) | (owner >= T)] == -1).all()


def test_owner_argument_checks_write_nothing(gpu_device):
    owner, ids = torch.zeros((2, 4, 4), dtype=torch.int8, device="cuda"), torch.zeros((3, 2), dtype=torch.int32, device="cuda")
    for kw, code in ((dict(owner=None), -1), (dict(ids=None), -1), (dict(out=None), -1), (dict(T=0), -2), (dict(T=33), -2), (dict(R=0), -2),
                     (dict(H=0), -2), (dict(W=-1), -2)):
        st, got, clean = run_owner(owner, ids, 3, **kw)
        assert st == code and clean and (got == 99).all(), kw


# ---- 3. air_track_score ---------------------------------------------------------------------------------------------------------------
def run_score(case, ids_host, gt_host, tau=0.5, **kw):
    from attend_infer_repeat_amd import hip as Hh
    T, S, F = case["T"], case["S"], case["F"]
    R, G = S * F, gt_host.shape[1]
    shapes = dict(seq_counts=((S, 8), torch.int32), seq_iou=((S,), torch.float64), gt_match=((R, G), torch.int32))
    bufs = {k: sentinel(*v) for k, v in shapes.items()}
    d = dict(boxes=dev_t(case["boxes"]), n=dev_t(case["n"].astype(np.int32)), ids=dev_t(ids_host.astype(np.int32)), gt=dev_t(gt_host))
    p = Hh._p
    a = dict(boxes=p(d["boxes"]), n=p(d["n"]), ids=p(d["ids"]), gt=p(d["gt"]), tau=tau, T=T, G=G, S=S, F=F, R=R)
    a.update({k: p(bufs[k][0]) for k in shapes})
    a.update(kw)
    st = Hh.lib().air_track_score(a["boxes"], a["n"], a["ids"], a["gt"], float(a["tau"]), a["T"], a["G"], a["S"], a["F"], a["R"],
                                  a["seq_counts"], a["seq_iou"], a["gt_match"], Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k, (shape, _) in shapes.items():
        n = int(np.prod(shape))
        got[k] = bufs[k][0][:n].view(shape).cpu().numpy()
        clean = clean and bool((bufs[k][0][n:] == bufs[k][1]).all())
    return st, got, clean, {k: bufs[k][1] for k in shapes}


@pytest.mark.parametrize("T,S,F,G,tau", [(3, 3, 5, 1, 0.5), (3, 3, 5, 8, 0.5), (6, 2, 17, 8, 0.3), (32, 1, 5, 8, 0.5), (1, 3, 2, 1, 0.0),
                                         (6, 3, 1, 3, 0.5)])
def test_score_is_the_reference(gpu_device, T, S, F, G, tau):
    case, ref = crafted_rows(T, 5, S, F, seed=T + S + F + G)
    rng = np.random.default_rng(T + G)
    gt = moving_gt(case, rng, G)
    ids = ref["track_id"].copy()
    flip = rng.uniform(size=ids.shape) < 0.1                       # identity switches the association did not make
    ids[flip & (ids >= 0)] += 1
    assert (gt[..., 2] <= 0).any() and (gt[..., 2] > 0).any()      # absent ground-truth rows included
    want = track.reference_score(case["boxes"], case["n"], ids, gt, F, tau)
    st, got, clean, _ = run_score(case, ids, gt, tau)
    assert st == 0 and clean
    assert np.array_equal(got["seq_counts"], want["seq_counts"]), (got["seq_counts"], want["seq_counts"])
    assert np.array_equal(got["gt_match"], want["gt_match"])
    assert np.all(np.abs(got["seq_iou"] - want["seq_iou"]) <= 1e-12 * np.abs(want["seq_iou"]))
    print("counts", want["seq_counts"].sum(0).tolist())
    assert want["seq_counts"][:, 0].sum() > 0


def test_score_argument_checks_write_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case, ref = crafted_rows(3, 5, 2, 4, seed=8)
    gt = moving_gt(case, np.random.default_rng(0), 2)
    off = torch.zeros(2 * 8 * 4 + 1, device="cuda")
    for kw, code in ((dict(boxes=None), -1), (dict(ids=None), -1), (dict(gt=None), -1), (dict(seq_iou=None), -1), (dict(T=0), -2),
                     (dict(T=33), -2), (dict(G=0), -2), (dict(G=9), -2), (dict(S=0), -2), (dict(F=0), -2), (dict(R=9), -2),
                     (dict(tau=-0.1), -2), (dict(tau=1.5), -2), (dict(tau=float("nan")), -2), (dict(gt=Hh._p(off[1:])), -3)):
        st, got, clean, fill = run_score(case, ref["track_id"], gt, **kw)
        assert st == code, kw
        assert clean and all((got[k] == fill[k]).all() for k in got), kw


# ---- 4. SequenceTracker ---------------------------------------------------------------------------------------------------------------
def make_tracker(name, S, F, provider="scene", capture=False, **kw):
    from attend_infer_repeat_amd.prune import ParsePruner
    from attend_infer_repeat_amd.track import SequenceTracker
    ocfg, _, params, _ = e2e_case(name)
    ps = make_parser(ocfg, S * F, params)
    pr = ps if provider == "scene" else ParsePruner(ps, "present")
    tk = SequenceTracker(pr, F, **kw)
    if capture:
        ps.capture()
        if pr is not ps:
            pr.capture()
        tk.capture()
    return ocfg, tk, pr


def frames_for(ocfg, S, F, seed):
    """S sequences of F frames: a synthetic batch per sequence start, its objects shifted a pixel per frame (np.roll)"""
    from oracle import air_oracle as O
    base = O.synthetic_batch(ocfg, S, seed=seed)[0]
    return torch.stack([torch.roll(base, shifts=(f, f // 2), dims=(1, 2)) for f in range(F)], 1).contiguous()


def host_rows(base, T, R):
    return dict(what=base["what"].cpu().numpy().reshape(T, R, -1), boxes=base["boxes"].cpu().numpy(), score=base["score"].cpu().numpy(),
                n=base["num_objects"].cpu().numpy())


@pytest.mark.parametrize("name,provider,S,F", [("tiny", "scene", 3, 5), ("rect_t5", "scene", 2, 4), ("tiny", "scene", 4, 1),
                                               ("tiny", "prune", 3, 5)])
def test_tracker_is_provider_then_association(gpu_device, name, provider, S, F):
    ocfg, tk, pr = make_tracker(name, S, F, provider, iou_gate=0.05, birth_score=0.0)       # (an untrained model's scores are low)
    T, R = ocfg.max_steps, S * F
    assert (tk.T, tk.R, tk.S, tk.F) == (T, R, S, F) and tk.engine is pr.engine
    frames = frames_for(ocfg, S, F, seed=21)
    counts = torch.from_numpy(np.random.default_rng(9).integers(0, T + 1, R).astype(np.int32)).cuda()       # (random weights: the count
    out = tk.track(frames.cuda(), counts)                          #  head's own answer may be 0 everywhere)
    tk.synchronize()
    got = {k: v.clone() if torch.is_tensor(v) else v for k, v in out.items()}
    base = pr.parse(frames.reshape(R, *ocfg.img_size).cuda(), counts)
    pr.synchronize()
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8) if t.is_floating_point() else t
    for k in base:                                                 # the provider's result is what a plain parse() gives, bit for bit
        assert torch.equal(raw(got[k]), raw(base[k])) if torch.is_tensor(base[k]) else got[k] == base[k], k
    rows = host_rows(base, T, R)
    assert rows["n"].max() > 0 or provider == "prune"
    ref = track.reference_associate(rows["what"], rows["boxes"], rows["score"], rows["n"], F, iou_gate=0.05, birth_score=0.0,
                                    return_margins=True)
    safe = (ref["gate_margin"] >= MARGIN) & (ref["round_margin"] >= MARGIN)
    print("sequences inside the margins: %d of %d; tracks %s; states %s" % (safe.sum(), S, ref["num_tracks"].tolist(),
                                                                           ref["state_counts"].sum(0).tolist()))
    assert safe.sum() >= S - 1                                     # (a decision within rounding of flipping proves nothing either way)
    in_rows = np.repeat(safe, F)
    for k in OUTPUTS:
        g, want = got[k].cpu().numpy(), ref[k]
        g, want = (g[:, in_rows], want[:, in_rows]) if k in OUTPUTS[:5] else (g[safe], want[safe])
        assert np.array_equal(bits(g), bits(want)) if k == "affinity" else np.array_equal(g, want), k
    assert ref["num_tracks"].sum() > 0 or provider == "prune"       # (the subset search may empty every frame of a random model)
    owner = base["owner"].cpu().numpy()
    assert np.array_equal(got["track_owner"].cpu().numpy(), owner_reference(owner, got["track_id"].cpu().numpy(), T))
    assert got["track_owner"].dtype == torch.int16 and set(got) == set(base) | set(OUTPUTS) | {"track_owner"}
    assert tk.launch_count()["track_associate"] == 1 and list(tk.segments) == ["associate", "owner"]


def test_graph_replay_equals_eager_and_sequences_permute(gpu_device):
    S, F = 3, 5
    ocfg, eager, _ = make_tracker("rect_t5", S, F, birth_score=0.0)
    _, graph, _ = make_tracker("rect_t5", S, F, capture=True, birth_score=0.0)
    assert graph._graph is not None and eager._graph is None
    keys = OUTPUTS + ("track_owner", "num_objects", "boxes", "owner")
    first = None
    for seed in (31, 32, 31):
        frames = frames_for(ocfg, S, F, seed).cuda()
        a, b = eager.track(frames), graph.track(frames)
        eager.synchronize(); graph.synchronize()
        for k in keys:
            assert torch.equal(a[k], b[k]), k
        first = first or {k: b[k].clone() for k in keys}
    assert all(torch.equal(first[k], b[k]) for k in keys)           # nothing of the call in between is remembered
    assert first["num_tracks"].sum() > 0
    perm = [2, 0, 1]
    c = graph.track(frames[perm])
    graph.synchronize()
    rows = np.concatenate([np.arange(s * F, (s + 1) * F) for s in perm])
    for k in ("track_id", "obj_state", "affinity", "prev_frame", "prev_slot"):
        assert torch.equal(c[k], first[k][:, rows]), k
    for k in ("num_tracks", "track_first", "track_last", "track_length", "track_gaps", "state_counts"):
        assert torch.equal(c[k], first[k][perm]), k
    assert torch.equal(c["track_owner"], first["track_owner"][rows])
    graph.release_graphs()


def test_totals_accumulate_and_reset(gpu_device):
    S, F, G = 3, 5, 2
    ocfg, tk, pr = make_tracker("rect_t5", S, F, capture=True, birth_score=0.0)
    T, R = ocfg.max_steps, S * F
    frames = frames_for(ocfg, S, F, 31).cuda()
    out = tk.track(frames)
    tk.synchronize()
    rows = host_rows(out, T, R)
    case = dict(boxes=rows["boxes"], n=rows["n"], T=T, S=S, F=F)
    gt = moving_gt(case, np.random.default_rng(1), G).reshape(S, F, G, 4)
    want = track.reference_score(rows["boxes"], rows["n"], out["track_id"].cpu().numpy(), gt, F, 0.5)
    a = tk.score(torch.from_numpy(gt), accumulate=False)
    tk.synchronize()
    assert np.array_equal(a["seq_counts"].cpu().numpy(), want["seq_counts"]) and np.array_equal(a["gt_match"].cpu().numpy(), want["gt_match"])
    assert np.allclose(a["seq_iou"].cpu().numpy(), want["seq_iou"], rtol=1e-12, atol=0)
    once = tk.summary()
    same = lambda p, q: set(p) == set(q) and all(p[k] == q[k] or (np.isnan(p[k]) and np.isnan(q[k])) for k in p)
    assert same(once, track.mot_summary(want["seq_counts"].sum(0), float(a["totals_f"][0])))
    assert once["gt"] == int((gt[..., 2] > 0).sum()) > 0
    tk.score(torch.from_numpy(gt).cuda(), accumulate=True)
    twice = tk.summary()
    for k in ("gt", "matches", "misses", "false_positives", "id_switches", "gt_objects"):
        assert twice[k] == 2 * once[k], k
    assert (np.isnan(twice["mota"]) and np.isnan(once["mota"])) or twice["mota"] == once["mota"]
    tk.score(torch.from_numpy(gt), tau=0.3, accumulate=False)      # another threshold: a plan of its own, the totals restart
    assert tk.summary()["gt"] == once["gt"] and len(tk._score) == 2
    tk.reset()
    empty = tk.summary()
    assert empty["gt"] == 0 and np.isnan(empty["mota"]) and np.isnan(empty["motp"])
    with pytest.raises(ValueError, match="gt_boxes"):
        tk.score(torch.zeros(R + 1, G, 4))
    tk.release_graphs()


def test_refusals(gpu_device):
    import types
    from attend_infer_repeat_amd.track import SequenceTracker
    ocfg, _, params, _ = e2e_case("tiny")
    ps = make_parser(ocfg, 10, params)
    with pytest.raises(ValueError, match="multiple"):
        SequenceTracker(ps, 3)
    with pytest.raises(ValueError, match="iou_gate"):
        SequenceTracker(ps, 5, iou_gate=1.0)
    with pytest.raises(ValueError, match="ParticleParser"):
        SequenceTracker(types.SimpleNamespace(KIND="particle", engine=ps.engine, R=10, T=3), 5)
    tk = SequenceTracker(ps, 5)
    with pytest.raises(ValueError, match="frames"):
        tk.track(torch.zeros(5, 2, *ocfg.img_size).cuda())


def test_tracker_binds_to_a_tiled_parser(gpu_device):
    """a TiledSceneParser is a provider like the others: its merged scene rows are the frames' objects"""
    from test_tile import make_tiled, scenes_for
    from attend_infer_repeat_amd.track import SequenceTracker
    S, F = 2, 2
    ocfg, tp, pr, scene = make_tiled("rect_t5", "scene", S * F)
    tk = SequenceTracker(tp, F, iou_gate=0.05, birth_score=0.0)
    assert (tk.T, tk.R, tk.img_size) == (tp.T, S * F, scene)
    scenes = scenes_for(ocfg, scene, S * F, seed=21)
    counts = torch.from_numpy(np.random.default_rng(9).integers(0, ocfg.max_steps + 1, pr.R).astype(np.int32)).cuda()
    out = tk.track(scenes.reshape(S, F, *scene).cuda(), counts)      # (given counts per window: random weights may see nothing)
    tk.synchronize()
    n = out["num_objects"].cpu().numpy()
    assert n.max() > 0
    what, boxes, score = (out[k].cpu().numpy().copy() for k in ("what", "boxes", "score"))
    for r in range(S * F):                                         # rows beyond the count are not written by the merge: never read
        what[n[r]:, r], boxes[n[r]:, r], score[n[r]:, r] = 0, 0, 0
    ref = track.reference_associate(what, boxes, score, n, F, iou_gate=0.05, birth_score=0.0, return_margins=True)
    safe = (ref["gate_margin"] >= MARGIN) & (ref["round_margin"] >= MARGIN)
    print("sequences inside the margins: %d of %d; tracks %s" % (safe.sum(), S, ref["num_tracks"].tolist()))
    assert safe.any() and ref["num_tracks"].sum() > 0
    in_rows = np.repeat(safe, F)
    for k in OUTPUTS:
        g, want = out[k].cpu().numpy(), ref[k]
        g, want = (g[:, in_rows], want[:, in_rows]) if k in OUTPUTS[:5] else (g[safe], want[safe])
        assert np.array_equal(bits(g), bits(want)) if k == "affinity" else np.array_equal(g, want), k
    assert np.array_equal(out["track_owner"].cpu().numpy(), owner_reference(out["owner"].cpu().numpy(), out["track_id"].cpu().numpy(), tk.T))


# ---- 5. surface -----------------------------------------------------------------------------------------------------------------------
def test_track_on_the_model_does_not_disturb_training(gpu_device):
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    B, S, F, T = 8, 2, 4, 3
    air, ts, x, y = _mnist_air(B)
    twin, ts_twin, _, _ = _mnist_air(B)
    for _ in range(2):
        ts(); ts_twin()
    d = procedural_moving_mnist(S, F, n_objects=(1, 2), seed=3, n_templates=32, return_annotations=True)
    frames = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    before, obs_before = _train_state(air._engine), air.obs
    out = air.track(frames)
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert air.obs is obs_before and air._engine.global_step == 2 and air.tracked is out
    R = S * F
    shapes = {"track_id": (T, R), "obj_state": (T, R), "affinity": (T, R), "prev_frame": (T, R), "prev_slot": (T, R), "num_tracks": (S,),
              "track_first": (S, F * T), "track_last": (S, F * T), "track_length": (S, F * T), "track_gaps": (S, F * T),
              "state_counts": (S, 6), "track_owner": (R, 50, 50), "boxes": (T, R, 4), "owner": (R, 50, 50), "num_objects": (R,)}
    assert {k: tuple(out[k].shape) for k in shapes} == shapes
    assert (out["state_counts"].sum(1) == T * F).all() and out["track_owner"].dtype == torch.int16
    tk = air.tracker(S, F)
    assert tk is air.tracker(S, F) and tk._graph is not None and len(air._trackers) == 1
    assert torch.equal(tk.engine.flat_params, air._engine.flat_params) and int(tk.engine.step_dev.item()) == 2
    first = {k: out[k].clone() for k in shapes}
    again = air.track(frames)
    assert all(torch.equal(first[k], again[k]) for k in shapes)
    ts(); ts_twin()
    air._engine.synchronize(); twin._engine.synchronize()
    assert torch.equal(air._engine.flat_params, twin._engine.flat_params) and torch.equal(air._engine.rng_state, twin._engine.rng_state)
    # other arguments are other cached trackers; a third one drops the least recently used
    air.track(frames, max_age=0)
    assert len(air._trackers) == 2 and air.tracker(S, F, max_age=0).max_age == 0
    scores, tracker = air.score_track(frames, d["boxes"], accumulate=False, gt_instances=d["instances"], prune="present")
    assert len(air._trackers) == 2 and tracker is air.tracker(S, F, prune="present") and tracker.provider is air.track_scorer.parser
    assert tuple(scores["seq_counts"].shape) == (S, 8) and tuple(scores["gt_match"].shape) == (R, 2)
    assert tuple(scores["detection"]["box_iou"].shape) == (R, T, 2)
    summary, det = tracker.summary(), air.track_scorer.summary()
    assert summary["gt"] == int((d["boxes"][..., 2] > 0).sum()) == det["objects_gt"] and det["images"] == R
    assert summary["matches"] + summary["misses"] == summary["gt"]
    air.score_track(frames, d["boxes"], accumulate=True, gt_instances=d["instances"], prune="present")
    assert tracker.summary()["gt"] == 2 * summary["gt"] and air.track_scorer.summary()["images"] == 2 * R
    tracker.reset()
    assert tracker.summary()["gt"] == 0
    with pytest.raises(ValueError, match="frames"):
        air.track(frames[0])
    assert air.obs is obs_before


def test_make_track_fig(gpu_device, tmp_path):
    pytest.importorskip("matplotlib")
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    from attend_infer_repeat_amd.evaluation import make_track_fig
    air, ts, x, y = _mnist_air(8)
    d = procedural_moving_mnist(2, 3, n_objects=(1, 2), seed=5, n_templates=32)
    frames = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    fig = make_track_fig(frames, air.track(frames), 2, str(tmp_path), 7)
    assert fig is not None and os.path.getsize(os.path.join(tmp_path, "track_fig_7.png")) > 0


def test_training_script_track_eval_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--track-eval", "4:2.5"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_track_score"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count(" track score ") == 2
    for l in rec:
        assert l["n_frames"] == 4 and l["frames"] == 64 and l["gt"] > 0 and l["matches"] + l["misses"] == l["gt"]
        assert l["iou_gate"] == track.DEFAULTS["iou_gate"] and l["max_age"] == track.DEFAULTS["max_age"]
        states = [l["track_" + k] for k in track.STATES[1:]]
        assert all(v >= 0 for v in states) and sum(states) <= 64 * 3 and l["track_born"] == l["tracks"]
        assert l["track_matched"] + l["track_born"] >= 0 and (l["mota"] <= 1.0 or np.isnan(l["mota"]))
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-eval", "0"])
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-eval", "4:fast"])
