"""GPU tests of the temporal proposals (attend_infer_repeat_amd/temporal.py, csrc/temporal_kernels.hip).

air_temporal_pool alone is compared EXACTLY against temporal.reference_pool: every copy, state, source and decision; the float64 box IoU
uses only differences, products, sums and one division, so device and numpy agree to the bit (as air_track_associate does).  Joints and
band shares use test_engine.py's OUT_TOL / OUT_L2, as tests/test_propose.py does; a decision is compared against the rule run on the
device's own joints, and on the planted sequence, whose float64 winner leads by more than 2 * OUT_TOL * max|J| (asserted by
tests/test_temporal_host.py on the same case), against float64 directly."""
import types

import numpy as np
import pytest
import torch

import temporal_cases as tc
from temporal_cases import PLANTED, PRIORS, chain, planted_reference, planted_sequence, pool_rows
from test_engine import OUT_L2, OUT_TOL, check_tensor
from test_parse import MASK_THRESHOLD, SENTINEL_F, SENTINEL_I, _mnist_air, e2e_case, make_parser, run_objects, run_render
from test_prune import MULT, STD, cpu, dev_t, f64_layers, run_score, run_select
from test_refine import mixed_counts, same_bits
from test_track import frames_for

from attend_infer_repeat_amd import prune, temporal, track
from attend_infer_repeat_amd.temporal import ABSENT, DUPLICATE, FULL, KNOWN, NONFINITE, TAKEN

pytestmark = pytest.mark.gpu

TAIL = 16
bits = lambda a: np.ascontiguousarray(a).view(np.uint32) if np.asarray(a).dtype == np.float32 else np.ascontiguousarray(a)
np_ = lambda t: t.detach().cpu().numpy()


def test_the_shared_bars_are_the_engine_suites():
    assert (tc.OUT_TOL, tc.OUT_L2, tc.MULT, tc.STD) == (OUT_TOL, OUT_L2, MULT, STD)


# ---- 1. air_temporal_pool alone ---------------------------------------------------------------------------------------------------------
POOL_OUT = dict(what=("f4", lambda T, P, R, A, G: (T + P, R, A)), where=("f4", lambda T, P, R, A, G: (T + P, R, 4)),
                glimpse=("f4", lambda T, P, R, A, G: (T + P, R, G)), score=("f4", lambda T, P, R, A, G: (T + P, R)),
                presence=("f4", lambda T, P, R, A, G: (T + P, R)), source=("i4", lambda T, P, R, A, G: (T + P, R)),
                prior=("f8", lambda T, P, R, A, G: (T + P + 1,)), cand_state=("i1", lambda T, P, R, A, G: (R, 2 * T)),
                taken=("i4", lambda T, P, R, A, G: (R,)), partner=("i4", lambda T, P, R, A, G: (P, R)))
TORCH_DT = {"f4": torch.float32, "i4": torch.int32, "f8": torch.float64, "i1": torch.int8}
FILL = {"f4": SENTINEL_F, "i4": SENTINEL_I, "f8": SENTINEL_F, "i1": 99}


def run_pool(case, T, P, S, F, img, iou_novel=0.3, both_sides=1, interpolate=1, rnd=0, use_counts=True, source_in=None, offset=0,
             drop=(), misalign=(), sizes=None):
    """air_temporal_pool alone on device copies of `case` (current stream).  Every output is a flat sentinel fill with a tail; with
    offset=1 every float buffer of rows starts one float into its allocation (4-byte but not 16-byte aligned).  Returns (outputs as
    host arrays, status, True when everything beyond the outputs is still the sentinel)."""
    from attend_infer_repeat_amd import hip as Hh
    R, A, G = S * F, case["what"].shape[2], case["glimpse"].shape[2]
    shift = lambda a: torch.cat([torch.zeros(offset), torch.from_numpy(np.ascontiguousarray(a)).reshape(-1), torch.zeros(4)]).cuda()
    d = {k: shift(case[k]) for k in ("what", "where", "glimpse", "score")}
    d["presence"] = None if use_counts else dev_t(chain(np.clip(case["n"], 0, T), T))
    d["counts"] = dev_t(np.asarray(case["n"], np.int32)) if use_counts else None
    d["source_in"] = None if source_in is None else dev_t(np.asarray(source_in, np.int32))
    d["prior"] = dev_t(np.asarray(case["prior"], np.float64))
    out, shapes = {}, {}
    for k, (dt, shape) in POOL_OUT.items():
        shapes[k] = shape(T, P, R, A, G)
        out[k] = torch.full((offset + int(np.prod(shapes[k])) + TAIL,), FILL[dt], dtype=TORCH_DT[dt]).cuda()
    p = Hh._p
    off_in = lambda k: None if k in drop else (p(d[k][offset:]) if k in ("what", "where", "glimpse", "score") else p(d[k]))
    off_out = lambda k: None if k in drop else p(out[k][(1 if k in misalign else offset if POOL_OUT[k][0] == "f4" else 0):])
    t, pp, s, f, a, g, h, w = sizes or (T, P, S, F, A, G, img[0], img[1])
    st = Hh.lib().air_temporal_pool(off_in("what"), off_in("where"), off_in("glimpse"), off_in("score"), off_in("presence"), off_in("counts"),
                                    off_in("source_in"), off_in("prior"), rnd, t, pp, s, f, a, g, h, w, float(iou_novel), int(both_sides),
                                    int(interpolate), off_out("what"), off_out("where"), off_out("glimpse"), off_out("score"),
                                    off_out("presence"), off_out("source"), off_out("prior"), off_out("cand_state"), off_out("taken"),
                                    off_out("partner"), Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k, (dt, _) in POOL_OUT.items():
        o = offset if dt == "f4" else 0
        n = int(np.prod(shapes[k]))
        got[k] = out[k][o:o + n].reshape(shapes[k]).cpu().numpy()
        clean = clean and bool((out[k][:o] == FILL[dt]).all()) and bool((out[k][o + n:] == FILL[dt]).all())
    got["untouched"] = all(bool((v == FILL[POOL_OUT[k][0]]).all()) for k, v in out.items())
    return got, st, clean


def assert_pool_equal(got, ref, label):
    for k in POOL_OUT:
        assert np.array_equal(bits(got[k]), bits(ref[k])), (label, k)


@pytest.mark.parametrize("A,G", [(3, 9), (8, 16)])                 # the word copies / the 16-byte copies
@pytest.mark.parametrize("T,P", [(1, 1), (1, 2), (2, 4), (3, 3), (5, 1)])
def test_pool_matches_the_reference(gpu_device, T, P, A, G):
    S, img = 2, (24, 24)
    seen = set()
    for F in (1, 2, 3, 5):
        case = pool_rows(T, S, F, A, G, seed=T * 7 + F)
        R = S * F
        src = np.stack([np.random.default_rng(F).permutation(T + 9) for _ in range(R)], 1)[:T]
        for both, interp, rnd, source_in in ((1, 1, 0, None), (0, 1, 0, None), (1, 0, 2, src)):
            label = "T%d_P%d_F%d_both%d_mid%d" % (T, P, F, both, interp)
            ref = temporal.reference_pool(case["what"], case["where"], case["glimpse"], case["score"], case["n"], case["prior"], F, img, P,
                                          0.3, bool(both), bool(interp), round=rnd, source_in=source_in)
            got, st, clean = run_pool(case, T, P, S, F, img, 0.3, both, interp, rnd, True, source_in)
            assert st == 0 and clean, label
            assert_pool_equal(got, ref, label)
            seen |= set(got["cand_state"].reshape(-1).tolist())
            if F == 1:
                assert (got["cand_state"] == ABSENT).all() and (got["taken"] == 0).all() and np.isnan(got["what"][T:]).all()
        # a presence chain instead of the counts: the same bits
        chained, st, clean = run_pool(case, T, P, S, F, img, 0.3, 1, 0, 2, False, src)
        assert st == 0 and clean
        assert_pool_equal(chained, got, "chain_F%d" % F)
    print("temporal pool T=%d P=%d A=%d G=%d: states seen %s" % (T, P, A, G, sorted(seen)))
    assert {ABSENT, TAKEN} <= seen


def test_pool_with_buffers_offset_by_one_float_takes_the_word_path(gpu_device):
    T, P, S, F, A, G, img = 2, 4, 2, 3, 8, 16, (24, 24)            # vector-sized rows, buffers that are not 16-byte aligned
    case = pool_rows(T, S, F, A, G, seed=3)
    ref = temporal.reference_pool(case["what"], case["where"], case["glimpse"], case["score"], case["n"], case["prior"], F, img, P)
    got, st, clean = run_pool(case, T, P, S, F, img, offset=1)
    assert st == 0 and clean
    assert_pool_equal(got, ref, "offset")
    aligned, st, _ = run_pool(case, T, P, S, F, img)
    assert st == 0
    assert_pool_equal(aligned, got, "aligned")


def test_pool_reaches_every_state_on_the_device(gpu_device):
    seen = set()
    for T, P, S, F in ((2, 4, 2, 5), (3, 3, 2, 3), (5, 1, 3, 2), (1, 2, 2, 5)):       # test_temporal_host.py: these reach all six
        case = pool_rows(T, S, F, 3, 4, seed=T * 7 + F)
        for both in (1, 0):
            ref = temporal.reference_pool(case["what"], case["where"], case["glimpse"], case["score"], case["n"], case["prior"], F, (24, 24),
                                          P, 0.3, bool(both), True, round=1)
            got, st, clean = run_pool(case, T, P, S, F, (24, 24), 0.3, both, 1, 1)
            assert st == 0 and clean
            assert_pool_equal(got, ref, (T, P, S, F, both))
            seen |= set(got["cand_state"].reshape(-1).tolist())
    assert seen == {ABSENT, TAKEN, KNOWN, DUPLICATE, FULL, NONFINITE}


def test_pool_is_strict_at_the_bar(gpu_device):
    """IoU exactly 1 / 3 (test_temporal_host.py works the case): not KNOWN at the bar, KNOWN one ulp below it"""
    T, F = 1, 2
    where = np.array([[(0.5, 0.0, 0.5, 0.0), (0.5, 0.5, 0.5, 0.0)]], np.float32)
    case = dict(what=np.ones((T, F, 3), np.float32), where=where, glimpse=np.ones((T, F, 4), np.float32),
                score=np.full((T, F), 0.5, np.float32), n=np.array([1, 1]), prior=np.array([0.5, 0.5]))
    third = 32.0 / 96.0
    for thr, want in ((third, TAKEN), (np.nextafter(third, 0.0), KNOWN), (float("nan"), TAKEN)):
        got, st, _ = run_pool(case, T, 1, 1, F, (16, 16), iou_novel=thr)
        assert st == 0 and got["cand_state"][1].tolist() == [want, ABSENT] and got["cand_state"][0].tolist() == [ABSENT, want], thr


def test_pool_argument_checks_return_their_code_and_write_nothing(gpu_device):
    T, P, S, F, A, G, img = 2, 2, 2, 3, 4, 4, (8, 8)
    case = pool_rows(T, S, F, A, G, seed=1)
    ok = (T, P, S, F, A, G, 8, 8)
    change = lambda **kw: tuple(kw.get(k, v) for k, v in zip("TPSFAGHW", ok))
    for sizes in (change(T=0), change(T=7), change(T=6, P=1), change(P=0), change(P=5), change(T=1, P=3), change(T=5, P=2), change(S=0),
                  change(F=0), change(A=0), change(G=0), change(H=0), change(W=-1), change(S=1 << 16, F=1 << 15)):
        got, st, _ = run_pool(case, T, P, S, F, img, sizes=sizes)
        assert st == -2 and got["untouched"], sizes                # AIR_E_SHAPE
    got, st, _ = run_pool(case, T, P, S, F, img, rnd=-1)
    assert st == -2 and got["untouched"]
    for drop in (("what",), ("where",), ("glimpse",), ("score",), ("prior",), ("counts",), ("taken",), ("partner",), ("cand_state",),
                 ("source",)):
        got, st, _ = run_pool(case, T, P, S, F, img, drop=drop)
        assert st == -1 and got["untouched"], drop                 # AIR_E_NULL (counts dropped: neither form is given)
    got, st, _ = run_pool(case, T, P, S, F, img, drop=("counts",), use_counts=False)
    assert st == 0                                                 # the chain alone is fine
    from attend_infer_repeat_amd import hip as Hh
    p = Hh._p
    f = torch.zeros(256).cuda()
    raw = f.view(torch.uint8)
    o = torch.full((256,), SENTINEL_F).cuda()
    i32, i8 = torch.full((64,), SENTINEL_I, dtype=torch.int32).cuda(), torch.full((64,), 99, dtype=torch.int8).cuda()
    d8 = torch.full((16,), SENTINEL_F, dtype=torch.float64).cuda()
    call = lambda **kw: Hh.lib().air_temporal_pool(kw.get("what", p(f)), p(f), p(f), p(f), None, p(i32.clone().zero_()), None,
                                                   kw.get("prior", p(d8.clone())), 0, T, P, S, F, A, G, 8, 8, 0.3, 1, 1, p(o), p(o), p(o),
                                                   kw.get("score", p(o)), p(o), p(i32), kw.get("pool_prior", p(d8)), p(i8), p(i32), p(i32),
                                                   Hh._stream())
    assert call(what=p(raw[2:])) == -3 and call(score=p(o.view(torch.uint8)[1:])) == -3      # AIR_E_ALIGN: not 4-byte aligned
    assert call(prior=p(d8.view(torch.float32)[1:])) == -3 and call(pool_prior=p(d8.view(torch.float32)[1:])) == -3      # float64: 8 bytes
    torch.cuda.synchronize()
    assert (o == SENTINEL_F).all() and (i32 == SENTINEL_I).all() and (i8 == 99).all() and (d8 == SENTINEL_F).all()


# ---- 2. the planted sequence through the entries ----------------------------------------------------------------------------------------
def through_the_entries(case, interpolate, both_sides=1):
    """air_temporal_pool -> air_prune_score -> air_prune_select (T := C) -> air_propose_source"""
    from attend_infer_repeat_amd import hip as Hh
    T, P, F = PLANTED["T"], PLANTED["P"], PLANTED["F"]
    (H, W), (h, w) = PLANTED["img"], PLANTED["crop"]
    C, R = T + P, F
    pool, st, clean = run_pool(case, T, P, 1, F, (H, W), 0.3, both_sides, interpolate, 0, False)
    assert st == 0 and clean
    sc = dict(glimpse=pool["glimpse"].reshape(C, R, h, w), where=pool["where"], presence=pool["presence"], obs=case["obs"], img=(H, W),
              crop=(h, w), T=C, B=R)
    rec_sub, st = run_score(sc, 1)
    assert st == 0
    sel = dict(what=pool["what"], where=pool["where"], glimpse=pool["glimpse"], score=pool["score"], presence=pool["presence"],
               where_loc=pool["where"], rec_sub=rec_sub.cpu().numpy())
    got, st = run_select(sel, PRIORS, pool["prior"], 1, 1)
    assert st == 0
    src = torch.full((C, R), SENTINEL_I, dtype=torch.int32).cuda()
    st = Hh.lib().air_propose_source(Hh._p(dev_t(pool["source"])), Hh._p(got["kept_step"]), C, R, Hh._p(src), Hh._stream())
    torch.cuda.synchronize()
    assert st == 0
    got["source_out"] = src
    return pool, rec_sub, got


@pytest.mark.parametrize("motion,interpolate", [(True, 1), (False, 0), (True, 0)])
def test_planted_sequence_through_the_entries(gpu_device, motion, interpolate):
    T, P, F = PLANTED["T"], PLANTED["P"], PLANTED["F"]
    C = T + P
    case = planted_sequence(motion)
    ref_pool, ref_rec, ref = planted_reference(case, bool(interpolate))
    pool, rec_sub, got = through_the_entries(case, interpolate)
    assert_pool_equal(pool, ref_pool, "planted")
    J = np_(got["J_sub"])
    finite = np.isfinite(ref["J_sub"])
    assert np.array_equal(np.isnan(J), np.isnan(ref["J_sub"])) and np.array_equal(np.isneginf(J), np.isneginf(ref["J_sub"]))
    assert np.isnan(J[0, 4:]).all() and np.isnan(J[2, 4:]).all()   # frames 0 and 2: every mask with the filler row
    check_tensor("temporal", "planted_motion%d_mid%d" % (motion, interpolate), "out", "J_sub", torch.from_numpy(J[finite]),
                 torch.from_numpy(ref["J_sub"][finite]), OUT_TOL, OUT_L2)
    order = np.sort(np.where(finite, ref["J_sub"], -np.inf), axis=1)[:, ::-1]
    bar = 2 * OUT_TOL * np.abs(ref["J_sub"][finite]).max()
    sure = order[:, 0] - order[:, 1] > bar
    print("planted (motion=%s, interpolate=%d): float64 leads %s, bar %.4g, device masks %s" % (
        motion, interpolate, (order[:, 0] - order[:, 1]).tolist(), bar, np_(got["best_mask"]).tolist()))
    if motion == bool(interpolate):                                # the two cases whose outcome the issue states
        assert sure.all() and ref["best_mask"].tolist() == [3, 0b101, 3]
    best, kept = np_(got["best_mask"]), np_(got["kept_step"])
    own = prune.reference_select(pool["what"], pool["where"], pool["glimpse"], pool["score"], pool["presence"], None, PRIORS, pool["prior"],
                                 1, 1, ref_rec, J_sub=J)           # the rule on the device's own joints: every frame
    assert np.array_equal(best, own["best_mask"]) and np.array_equal(kept, own["kept_step"])
    assert np.array_equal(best[sure], ref["best_mask"][sure]) and np.array_equal(kept[:, sure], ref["kept_step"][:, sure])
    assert (np_(got["objective"]) >= np_(got["objective_start"])).all()      # never worse
    for k in ("what", "where", "glimpse", "score"):                # the compacted rows are copies of the pool's
        g = np_(got[k + "_out"])
        assert np.array_equal(bits(g), bits(np.stack([pool[k][kept[:, r], r] for r in range(F)], 1))), k
    src = np_(got["source_out"])
    assert np.array_equal(src, np.take_along_axis(pool["source"], kept.astype(np.int64), 0))
    if motion == bool(interpolate):
        assert np_(got["num_objects_out"]).tolist() == [2, 2, 2] and src[:, 1].tolist() == [0, T + 1, 1]
        for r in (0, 2):                                           # frames 0 and 2 return their start parse unchanged
            assert kept[:, r].tolist() == [0, 1, 2] and np_(got["objective"])[r] == np_(got["objective_start"])[r]


# ---- 3. TemporalProposer behind the providers -------------------------------------------------------------------------------------------
def make_temporal(name, S, F, provider="scene", proposals=1, rounds=1, capture=False, **kw):
    from attend_infer_repeat_amd.propose import ParseProposer
    from attend_infer_repeat_amd.refine import ParseRefiner
    from attend_infer_repeat_amd.temporal import TemporalProposer
    ocfg, _, params, _ = e2e_case(name)
    stack = [make_parser(ocfg, S * F, params)]
    if provider == "refine":
        stack.append(ParseRefiner(stack[-1], 2, 1e-2, 1e-2))
    if provider == "propose":
        stack.append(ParseProposer(stack[-1], 1, 1))
        stack[-1].load_parameters(params)
        stack[-1].set_global_step(20000)
    stack.append(TemporalProposer(stack[-1], F, proposals, rounds, **kw))
    if capture:
        for s in stack:
            s.capture()
    return stack[-1], ocfg, params


def seq_counts(ocfg, S, F, seed=9):
    """given counts: the count head of a random model may say 0 everywhere; frames of a sequence differ, so neighbours hold more"""
    n = np.random.default_rng(seed).integers(0, ocfg.max_steps + 1, S * F).astype(np.int32)
    return torch.from_numpy(n).cuda()


def check_rounds(tp, ocfg, base, obs, out, label):
    """every round of one call: the pool against reference_pool on the round's input rows (exact), the joints against float64 fed with
    the device's own pool rows, the decision on the device's own joints, the provenance, and the round invariants"""
    from attend_infer_repeat_amd import propose
    T, R, P, C, Rn, F = tp.T, tp.R, tp.proposals, tp.C, tp.rounds, tp.F
    (H, W), (h, w) = ocfg.img_size, ocfg.crop_size
    mult, std = float(ocfg.output_multiplier), float(ocfg.output_std)
    priors = (*ocfg.what_prior, *ocfg.where_scale_prior, *ocfg.where_shift_prior)
    table = np_(tp.engine.prior_dev)
    obs_np = obs.reshape(R, H, W).numpy()
    cur = dict(what=np_(base["what"]), where=np_(base["where"]), glimpse=np_(base["glimpse"]).reshape(T, R, -1), score=np_(base["score"]))
    n = np_(base["num_objects"]).astype(np.int64)
    assert np.array_equal(np_(out["num_objects_start"]), n)
    src_in, kept_m0 = None, np.ones(R, bool)
    obj = np_(tp.objective_rounds)
    pop = np.array([bin(m).count("1") for m in range(1 << C)])
    for r in range(Rn):
        pool = {k: np_(getattr(tp, "pool_" + k)[r]) for k in ("what", "where", "glimpse", "score", "presence", "source")}
        ref_pool = temporal.reference_pool(cur["what"], cur["where"], cur["glimpse"], cur["score"], n, table, F, (H, W), P, tp.iou_novel,
                                           tp.direction == "both", tp.interpolate, round=r, source_in=src_in)
        for k in pool:
            assert np.array_equal(bits(pool[k]), bits(ref_pool[k])), (label, r, k)
        assert np.array_equal(np_(tp.pool_prior), ref_pool["prior"])
        assert np.array_equal(np_(out["cand_state"][r]), ref_pool["cand_state"]) and np.array_equal(np_(out["partner"][r]), ref_pool["partner"])
        assert np.array_equal(np_(out["proposals_taken"][r]), ref_pool["taken"])
        case = dict(glimpse=pool["glimpse"].reshape(C, R, h, w), where=pool["where"], img=(H, W), T=C)
        rec = prune.reference_score(case["glimpse"], case["where"], pool["presence"], obs_np, mult, std, 1, layers=f64_layers(case))
        sel_in = (pool["what"], pool["where"], pool["glimpse"], pool["score"], pool["presence"], None, priors, ref_pool["prior"], 1, 1, rec)
        ref = prune.reference_select(*sel_in)
        J = np_(tp.J_sub[r])
        finite = np.isfinite(ref["J_sub"])
        filler = (np.arange(C)[:, None] >= T + ref_pool["taken"][None, :])      # [C, R]
        has_filler = np.stack([[any(filler[j, b] for j in range(C) if (m >> j) & 1) for m in range(1 << C)] for b in range(R)], 0)
        assert np.array_equal(np.isnan(J), has_filler) and np.array_equal(np.isnan(ref["J_sub"]), has_filler)
        assert np.array_equal(np.isneginf(J), ~has_filler & np.broadcast_to(pop > T, J.shape))
        check_tensor("temporal", "%s_round%d" % (label, r), "out", "J_sub", torch.from_numpy(J[finite]), torch.from_numpy(ref["J_sub"][finite]),
                     OUT_TOL, OUT_L2)
        own = prune.reference_select(*sel_in, J_sub=J)             # the rule on the DEVICE's joints: exact, no frame left out
        assert np.array_equal(np_(tp.best_mask[r]), own["best_mask"]) and np.array_equal(np_(tp.kept_pool[r]), own["kept_step"])
        assert np.array_equal(np_(tp.num_objects_round[r]), own["num_objects"]) and (own["num_objects"] <= T).all()
        assert np.array_equal(obj[r + 1], own["objective"]) and np.array_equal(np_(tp.objective_start_rounds[r]), own["objective_start"])
        assert np.array_equal(np_(tp.evidence[r]), own["evidence"], equal_nan=True)
        for k in ("what", "where", "glimpse", "score"):
            assert np.array_equal(bits(np_(getattr(tp, "out_" + k)[r])), bits(own[k])), (r, k)
        src_out = propose.reference_source(pool["source"], own["kept_step"])
        assert np.array_equal(np_(tp.source_out[r]), src_out)
        kept_m0 &= own["best_mask"] == (1 << n) - 1
        states = np.bincount(ref_pool["cand_state"].reshape(-1), minlength=6).tolist()
        print("temporal %s round %d: n %s, states %s, taken %s -> best masks %s, objective gain max %.3g" % (
            label, r, n.tolist(), states, ref_pool["taken"].tolist(), [bin(m) for m in own["best_mask"]],
            float(np.nanmax(own["objective"] - own["objective_start"]))))
        cur = {k: own[k][:T] for k in ("what", "where", "glimpse", "score")}
        n, src_in = own["num_objects"], src_out
    assert (obj[1:] >= obj[:-1]).all()                             # never worse, round after round
    for r in range(1, Rn):
        assert np.array_equal(np_(tp.objective_start_rounds[r]), obj[r])      # bit for bit: the compaction keeps step order
    assert np.array_equal(np_(out["objective"]), obj[-1]) and np.array_equal(np_(out["objective_start"]), obj[0])
    assert np.array_equal(np_(out["kept_step"]), src_in[:T]) and np.array_equal(np_(out["num_objects"]), n)
    kept_rows = np.arange(T)[:, None] < n[None, :]
    assert np.array_equal(np_(out["objects_temporal_kept"]), ((src_in[:T] >= T) & kept_rows).sum(0))
    named = src_in[:T][(src_in[:T] >= T) & kept_rows] - T          # kept_step - T = round * 2T + q
    assert ((named // (2 * T)) < Rn).all()
    assert same_bits(out["proposal_what"], tp.pool_what[:, T:].cpu()) and tuple(out["proposal_glimpse"].shape) == (Rn, P, R, h, w)
    return n, kept_m0


def check_readout(tp, ocfg, out_dev, out, base, n, kept_m0):
    """the read-out against air_parse_objects / air_parse_render on the first T compacted rows, bit for bit; frames that kept their
    start mask in every round return the provider's parse bit for bit"""
    T, R = tp.T, tp.R
    (H, W), (h, w) = ocfg.img_size, ocfg.crop_size
    hand = run_objects(out_dev["presence_prob"], out_dev["num_objects"], out_dev["where"].contiguous(), out_dev["what"].contiguous(), H, W)
    for k in ("num_objects", "count_prob", "presence", "boxes", "offsets"):
        assert same_bits(out_dev[k], hand[k]), k
    rows = int(out["offsets"][-1])
    for k in ("obj_image", "obj_box", "obj_where", "obj_what"):
        assert same_bits(out_dev[k][:rows], hand[k][:rows]), k
    kept_rows = np.arange(T)[:, None] < n[None, :]
    score_src = np_(tp.out_score[-1, :T])
    assert np.array_equal(out["score"].numpy(), np.where(kept_rows, score_src, np_(hand["score"])), equal_nan=True)
    for b in range(R):
        lo, hi = int(out["offsets"][b]), int(out["offsets"][b + 1])
        assert hi - lo == n[b] and out["obj_step"][lo:hi].tolist() == out["kept_step"][:hi - lo, b].tolist()
    rend = run_render(out_dev["glimpse"].contiguous(), out_dev["where"].contiguous(), out_dev["presence"], tp._start["obs"].view(R, H, W),
                      float(ocfg.output_multiplier), float(ocfg.output_std), (H, W), (h, w), layers=False)
    for k in ("reconstruction", "owner", "area", "rec"):
        assert same_bits(out_dev[k], rend[k]), k
    for b in np.nonzero(kept_m0)[0]:
        assert_frame_equals_provider(out, base, b, T, R)
    return int(kept_m0.sum())


def assert_frame_equals_provider(out, base, b, T, R):
    for k in base:
        if k in ("offsets", "layers") or k in TEMPORAL_KEYS or k not in out:
            continue                                               # (behind another searcher the search's keys are that searcher's)
        if k == "obj_step" and "kept_step" in base:
            continue                                               # (... and its labels: ours index its compacted rows)
        v, u = out[k], base[k]
        if k.startswith("obj_"):
            assert same_bits(v[int(out["offsets"][b]):int(out["offsets"][b + 1])], u[int(base["offsets"][b]):int(base["offsets"][b + 1])]), k
        elif v.dim() > 1 and v.shape[0] == T and v.shape[1] == R:
            assert same_bits(v[:, b], u[:, b]), k
        elif v.dim() > 0 and v.shape[0] == R and u.shape == v.shape:
            assert same_bits(v[b], u[b]), k


def test_planted_sequences_through_the_module(gpu_device):
    """The bound provider's buffers are overwritten with two planted sequences of three 50 x 50 frames and the state a provider would
    have returned for them; the rounds then run eagerly, segment by segment.  Sequence 0: the second object moves, frames 0 and 2 hold
    it, frame 1 does not -- round 0 recovers it at the midpoint.  Sequence 1: the second object stands still and only frame 0 holds it
    -- round 0 carries it into frame 1, round 1 from there into frame 2: with rounds = 2 an object travels two frames."""
    S, F, P, Rn = 2, 3, 1, 2
    tp, ocfg, params = make_temporal("mnist_b8", S, F, "scene", P, Rn)
    T, R, C, (H, W), (h, w), A = tp.T, tp.R, tp.C, ocfg.img_size, ocfg.crop_size, ocfg.n_appearance
    assert (T, R, C) == (3, 6, 4)
    mult, std = float(ocfg.output_multiplier), float(ocfg.output_std)
    par, st = tp.parser, tp._start
    first = tp.parse(torch.zeros(R, H, W).cuda(), mixed_counts(ocfg, R))      # binds, fills presence_prob and the count table
    tp.synchronize(); torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    place_a, place_b, step, junk = (0.3, -0.5, 0.3, -0.5), np.array((0.3, 0.5, 0.3, 0.5), np.float32), np.array((0, 0.05, 0, 0.05), np.float32), \
        (0.1, 3.0, 0.1, 3.0)
    truth = np.stack([place_b + (f - 1) * step for f in range(F)] + [place_b] * F, 0)      # the second object's place in row r
    holds_b = [True, False, True, True, False, False]
    where = np.empty((T, R, 4), np.float32)
    where[:] = junk
    where[0] = place_a
    where[1, holds_b] = truth[holds_b]
    glimpse = np.ones((T, R, h, w), np.float32)
    glimpse[1] = 0.75
    what = np.broadcast_to((rng.normal(size=(T, 1, A)) * 0.3).astype(np.float32), (T, R, A)).copy()
    score = np.full((T, R), 0.9, np.float32)
    score[1, 2] = 0.7                                              # the frame-0 sighting ranks first
    n = np.array([2 if b else 1 for b in holds_b], np.int32)
    g64 = lambda v: np.full((R, h, w), v, np.float64)
    canvas = prune._st_write(g64(1.0), np.broadcast_to(np.array(place_a, np.float64), (R, 4)), (H, W)) + \
        prune._st_write(g64(0.75), truth.astype(np.float64), (H, W))
    obs = (mult * canvas).astype(np.float32)
    st["what"].copy_(dev_t(what)); st["where"].copy_(dev_t(where)); st["glimpse"].copy_(dev_t(glimpse).reshape(st["glimpse"].shape))
    st["obs"].copy_(dev_t(obs).reshape(st["obs"].shape))
    prov = run_objects(st["presence_prob"], dev_t(n), st["where"], st["what"], H, W)
    par.presence.copy_(prov["presence"]); par.score.copy_(dev_t(score)); par.num_objects.copy_(prov["num_objects"])
    torch.cuda.synchronize()
    for r in range(Rn):
        tp.run_segments(r, "pool", "score", "select", "source")
    tp.engine._replay_or_run(None, tp.readout)
    tp.synchronize(); torch.cuda.synchronize()
    out_dev = tp._result({k: first[k] for k in first if k not in TEMPORAL_KEYS})
    out = cpu(out_dev)
    # round by round: the states, and the float64 winner on the device's pool rows ahead by more than the bar
    priors = (*ocfg.what_prior, *ocfg.where_scale_prior, *ocfg.where_shift_prior)
    expect_state = [{1: [KNOWN, TAKEN, ABSENT, KNOWN, DUPLICATE, ABSENT], 4: [KNOWN, TAKEN, ABSENT, KNOWN, ABSENT, ABSENT],
                     5: [KNOWN, ABSENT, ABSENT, ABSENT, ABSENT, ABSENT]},
                    {1: [KNOWN, KNOWN, ABSENT, KNOWN, KNOWN, ABSENT], 4: [KNOWN, KNOWN, ABSENT, KNOWN, ABSENT, ABSENT],
                     5: [KNOWN, TAKEN, ABSENT, ABSENT, ABSENT, ABSENT]}]
    expect_mask = [[0b0011, 0b1001, 0b0011, 0b0011, 0b1001, 0b0001], [0b0011, 0b0011, 0b0011, 0b0011, 0b0011, 0b1001]]
    for r in range(Rn):
        for row, want in expect_state[r].items():
            assert out["cand_state"][r, row].tolist() == want, (r, row)
        pool = {k: np_(getattr(tp, "pool_" + k)[r]) for k in ("what", "where", "glimpse", "score", "presence")}
        rec = prune.reference_score(pool["glimpse"].reshape(C, R, h, w), pool["where"], pool["presence"], obs, mult, std, 1)
        ref = prune.reference_select(pool["what"], pool["where"], pool["glimpse"], pool["score"], pool["presence"], None, priors,
                                     np_(tp.pool_prior), 1, 1, rec)
        finite = np.isfinite(ref["J_sub"])
        order = np.sort(np.where(finite, ref["J_sub"], -np.inf), axis=1)[:, ::-1]
        bar = 2 * OUT_TOL * np.abs(ref["J_sub"][finite]).max()
        print("planted module round %d: float64 leads %s, bar %.4g" % (r, np.round(order[:, 0] - order[:, 1], 3).tolist(), bar))
        assert ref["best_mask"].tolist() == expect_mask[r] and (order[:, 0] - order[:, 1] > bar).all()
        assert np_(tp.best_mask[r]).tolist() == expect_mask[r]
        check_tensor("temporal", "planted_module_round%d" % r, "out", "J_sub", torch.from_numpy(np_(tp.J_sub[r])[finite]),
                     torch.from_numpy(ref["J_sub"][finite]), OUT_TOL, OUT_L2)
    assert out["partner"][0, 0].tolist() == [-1, 4, -1, -1, -1, -1] and out["proposals_taken"].tolist() == [[0, 1, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1]]
    mid = (0.5 * (truth[0].astype(np.float64) + truth[2].astype(np.float64))).astype(np.float32)
    assert np.array_equal(bits(np_(out["where"])[1, 1]), bits(mid)) and np.abs(mid - truth[1]).max() < 1e-7
    assert np.array_equal(bits(np_(out["where"])[1, 4]), bits(truth[3])) and np.array_equal(bits(np_(out["where"])[1, 5]), bits(truth[3]))
    kept = out["kept_step"].numpy()
    assert out["num_objects"].tolist() == [2] * R and out["num_objects_start"].tolist() == n.tolist()
    assert kept[:2].T.tolist() == [[0, 1], [0, T + 1], [0, 1], [0, 1], [0, T + 1], [0, T + 2 * T + 1]]      # kept_step - T = round * 2T + q
    assert out["objects_temporal_kept"].tolist() == [0, 1, 0, 0, 1, 1]
    obj = out["objective_rounds"].numpy()
    assert (obj[1:] >= obj[:-1]).all() and (obj[1, [1, 4]] > obj[0, [1, 4]]).all() and obj[2, 5] > obj[1, 5] and obj[1, 5] == obj[0, 5]
    assert np.array_equal(np_(tp.objective_start_rounds[1]), obj[1])
    for row in (0, 2, 3):                                          # these frames keep their start parse, bit for bit
        for k in ("what", "where", "glimpse"):
            assert same_bits(out[k][:2, row].reshape(2, -1), torch.from_numpy({"what": what, "where": where, "glimpse": glimpse}[k])[:2, row].reshape(2, -1)), k
    assert np.abs(out["reconstruction"].numpy() - obs).max() <= OUT_TOL * np.abs(obs).max()
    for b in range(R):
        lo, hi = int(out["offsets"][b]), int(out["offsets"][b + 1])
        assert hi - lo == 2 and out["obj_step"][lo:hi].tolist() == kept[:2, b].tolist() and out["obj_score"][lo:hi].tolist()[0] == np.float32(0.9)
    check_readout(tp, ocfg, out_dev, out, {}, np.array([2] * R), np.zeros(R, bool))


TEMPORAL_KEYS = {"objective", "objective_start", "objective_subsets", "best_mask", "kept_step", "evidence", "num_objects_start",
                 "objective_rounds", "cand_state", "proposals_taken", "partner", "proposal_what", "proposal_where", "proposal_glimpse",
                 "proposal_score", "objects_temporal_kept"}


@pytest.mark.parametrize("provider,proposals,rounds", [("scene", 1, 1), ("scene", 3, 2), ("refine", 2, 1), ("propose", 1, 2)])
def test_temporal_proposer_behind_the_providers(gpu_device, provider, proposals, rounds):
    S, F = 2, 3
    tp, ocfg, params = make_temporal("tiny", S, F, provider, proposals, rounds)
    T, R = tp.T, tp.R
    assert (tp.S, tp.F, tp.R, tp.C) == (S, F, S * F, T + proposals) and tp.engine is tp.parser.engine
    frames = frames_for(ocfg, S, F, seed=21)
    obs = frames.reshape(R, *ocfg.img_size)
    counts = seq_counts(ocfg, S, F)
    base_dev = tp.parser.parse(obs.cuda(), counts)
    tp.synchronize()
    base = cpu(base_dev)
    out_dev = tp.parse(obs.cuda(), counts)
    tp.synchronize()
    torch.cuda.synchronize()
    out = cpu(out_dev)
    extra = {"refine": {"refine_objective", "refine_objective_start"}, "propose": {"provider_objective", "provider_objective_start"}}
    assert set(out) == set(base) | TEMPORAL_KEYS | extra.get(provider, set())
    label = "%s_P%d_R%d" % (provider, proposals, rounds)
    n, kept_m0 = check_rounds(tp, ocfg, base, obs, out, label)
    same = check_readout(tp, ocfg, out_dev, out, base, n, kept_m0)
    print("temporal %s: %d of %d frames kept their start mask throughout; %d objects came from a neighbour" % (
        label, same, R, int(out["objects_temporal_kept"].sum())))
    for k in ("presence_prob", "num_steps_posterior"):
        assert same_bits(out[k], base[k]), k
    assert tp.launch_count()["temporal_pool"] == rounds and len(tp._plan) == rounds * 4 + 4
    # the provider's buffers are only read: its parse is what it was
    again = cpu(tp.parser.parse(obs.cuda(), counts))
    tp.synchronize()
    assert all(same_bits(again[k], base[k]) for k in base)


def test_one_frame_per_sequence_returns_the_providers_parse(gpu_device):
    """F = 1: no neighbour exists, every proposal row is a filler row, and a round is the subset search over the frame's own rows.
    Behind a provider that has run that search already (a ParseProposer: its parse is a fixed point of it) every frame keeps its
    start mask and the result is the provider's parse, bit for bit."""
    S, F = 6, 1
    tp, ocfg, params = make_temporal("tiny", S, F, "propose", 2, 2)
    obs = frames_for(ocfg, S, F, seed=21).reshape(S, *ocfg.img_size)
    counts = seq_counts(ocfg, S, F)
    base = cpu(tp.parser.parse(obs.cuda(), counts))
    tp.synchronize()
    out = cpu(tp.parse(obs.cuda(), counts))
    tp.synchronize()
    assert (out["cand_state"] == ABSENT).all() and (out["proposals_taken"] == 0).all() and (out["objects_temporal_kept"] == 0).all()
    assert torch.isnan(out["proposal_what"]).all() and (out["proposal_score"] == 0).all()
    assert (out["kept_step"] == torch.arange(tp.T, dtype=torch.int32)[:, None]).all()
    assert same_bits(out["objective"], out["objective_start"]) and same_bits(out["offsets"], base["offsets"])
    for b in range(S):
        assert_frame_equals_provider(out, base, b, tp.T, S)
    for k in ("what", "where", "glimpse", "score", "boxes", "presence", "num_objects", "owner", "reconstruction", "rec", "area", "count_prob",
              "obj_image", "obj_box", "obj_score", "obj_where", "obj_what"):
        assert same_bits(out[k], base[k]), k


def test_one_frame_per_sequence_behind_a_scene_parser_is_the_subset_search(gpu_device):
    """F = 1 behind a provider that has NOT run the search: the filler rows are never taken, so the result is what ParsePruner("all")
    selects on the same rows -- the same masks and the same compacted rows"""
    from attend_infer_repeat_amd.prune import ParsePruner
    S, F = 6, 1
    tp, ocfg, params = make_temporal("tiny", S, F, "scene", 2, 1)
    pr = ParsePruner(tp.parser, "all")
    obs = frames_for(ocfg, S, F, seed=21).reshape(S, *ocfg.img_size)
    counts = seq_counts(ocfg, S, F)
    want = cpu(pr.parse(obs.cuda(), counts))
    pr.synchronize()
    out = cpu(tp.parse(obs.cuda(), counts))
    tp.synchronize()
    T = tp.T
    assert (out["cand_state"] == ABSENT).all() and ((out["best_mask"] >> T) == 0).all()
    assert torch.equal(out["best_mask"], want["best_mask"]) and torch.equal(out["kept_step"], want["kept_step"])
    for k in ("num_objects", "what", "where", "glimpse", "score", "boxes", "presence", "owner", "reconstruction", "area", "obj_step"):
        assert same_bits(out[k], want[k]), k
    check_tensor("temporal", "one_frame", "out", "objective", out["objective"], want["objective"], OUT_TOL, OUT_L2)
    assert torch.isnan(out["objective_subsets"][:, 1 << T:]).all()


def test_graph_replay_equals_eager_and_sequences_swap(gpu_device):
    S, F = 2, 3
    eager, ocfg, _ = make_temporal("tiny", S, F, "scene", 2, 2)
    graph, _, _ = make_temporal("tiny", S, F, "scene", 2, 2, capture=True)
    assert graph._graph is not None and eager._graph is None
    R = S * F
    first = None
    for seed in (31, 32, 31):
        obs = frames_for(ocfg, S, F, seed).reshape(R, *ocfg.img_size).cuda()
        counts = seq_counts(ocfg, S, F, seed=seed)
        a, b = eager.parse(obs, counts), graph.parse(obs, counts)
        eager.synchronize(); graph.synchronize(); torch.cuda.synchronize()
        assert set(a) == set(b)
        for k in a:
            assert same_bits(a[k], b[k]), k
        first = first or {k: v.clone() for k, v in b.items()}
    assert all(same_bits(first[k], b[k]) for k in first)           # nothing of the call in between is remembered
    rows = torch.cat([torch.arange(F, 2 * F), torch.arange(0, F)]).cuda()      # the two sequences swapped: R is the same, so is the banding
    c = graph.parse(obs[rows], counts[rows])
    graph.synchronize(); torch.cuda.synchronize()
    T = graph.T
    for k, v in c.items():
        u = first[k]
        if k in ("offsets",) or k.startswith("obj_"):
            continue                                               # (the table is image-major: compared through its rows below)
        if k in ("cand_state", "proposals_taken", "objective_rounds"):
            assert same_bits(v, u[:, rows]), k
        elif k in ("partner", "proposal_what", "proposal_where", "proposal_glimpse", "proposal_score"):
            assert same_bits(v, u[:, :, rows]), k
        elif v.dim() > 1 and v.shape[0] in (T, graph.C) and v.shape[1] == R:
            assert same_bits(v, u[:, rows]), k
        elif v.dim() > 0 and v.shape[0] == R:
            assert same_bits(v, u[rows]), k
        else:
            raise AssertionError("unexpected layout of %r: %s" % (k, tuple(v.shape)))
    for b in range(R):
        lo, hi, lo0 = int(c["offsets"][b]), int(c["offsets"][b + 1]), int(first["offsets"][int(rows[b])])
        for k in ("obj_step", "obj_box", "obj_score", "obj_where", "obj_what"):
            assert same_bits(c[k][lo:hi], first[k][lo0:lo0 + hi - lo]), k
    graph.release_graphs(); graph.parser.release_graphs()


def test_refusals(gpu_device):
    from attend_infer_repeat_amd.temporal import TemporalProposer
    ocfg, _, params, _ = e2e_case("tiny")
    ps = make_parser(ocfg, 10, params)
    with pytest.raises(ValueError, match="multiple"):
        TemporalProposer(ps, 3)
    with pytest.raises(ValueError, match="proposals"):
        TemporalProposer(ps, 5, 4)
    with pytest.raises(ValueError, match="direction"):
        TemporalProposer(ps, 5, direction="future")
    with pytest.raises(ValueError, match="ParticleParser"):
        TemporalProposer(types.SimpleNamespace(KIND="particle", engine=ps.engine, R=10, T=3), 5)
    with pytest.raises(ValueError, match="TiledSceneParser"):
        TemporalProposer(types.SimpleNamespace(KIND="tiled", engine=ps.engine, R=10, T=3), 5)
    past = TemporalProposer(ps, 5, direction="past", interpolate=False)
    out = past.parse(torch.zeros(10, *ocfg.img_size).cuda(), mixed_counts(ocfg, 10))
    past.synchronize()
    assert (out["cand_state"][:, :, past.T:] == ABSENT).all() and (out["partner"] == -1).all()


# ---- 4. bindings and the surface ----------------------------------------------------------------------------------------------------------
def test_tracker_and_scorer_bind_to_a_temporal_proposer(gpu_device):
    from test_track import MARGIN, host_rows
    from test_track_host import OUTPUTS
    from attend_infer_repeat_amd.score import ParseScorer
    from attend_infer_repeat_amd.track import SequenceTracker
    S, F, G = 2, 3, 2
    tp, ocfg, _ = make_temporal("tiny", S, F, "scene", 2, 1)
    T, R = tp.T, tp.R
    tk = SequenceTracker(tp, F, iou_gate=0.05, birth_score=0.0)
    sc = ParseScorer(tp, G)
    frames = frames_for(ocfg, S, F, seed=21)
    counts = seq_counts(ocfg, S, F)
    out = tk.track(frames.cuda(), counts)
    tk.synchronize()
    for k in ("what", "boxes", "score", "num_objects", "owner"):
        assert out[k].data_ptr() == getattr(tp, k).data_ptr(), k
    rows = host_rows(out, T, R)
    ref = track.reference_associate(rows["what"], rows["boxes"], rows["score"], rows["n"], F, iou_gate=0.05, birth_score=0.0,
                                    return_margins=True)
    safe = (ref["gate_margin"] >= MARGIN) & (ref["round_margin"] >= MARGIN)
    assert safe.sum() >= S - 1
    in_rows = np.repeat(safe, F)
    for k in OUTPUTS:
        g, want = np_(out[k]), ref[k]
        g, want = (g[:, in_rows], want[:, in_rows]) if k in OUTPUTS[:5] else (g[safe], want[safe])
        assert np.array_equal(bits(g), bits(want)), k
    rng = np.random.RandomState(2)
    H, W = ocfg.img_size
    gt_inst = torch.from_numpy(rng.randint(-1, G, (R, H, W)).astype(np.int8))
    gt_boxes = torch.from_numpy(np.tile(np.array([0.0, 0.0, W, H], np.float32), (R, G, 1)))
    s = sc.score(gt_inst, gt_boxes.cuda(), accumulate=False)
    summary = sc.summary()
    assert summary["images"] == R and np.isfinite(summary["count_acc"]) and torch.is_tensor(s["ari"])


def test_track_on_the_model_with_temporal(gpu_device):
    from attend_infer_repeat_amd.temporal import TemporalProposer
    air, ts, x, y = _mnist_air(8)
    ts()
    S, F = 2, 3
    frames = torch.stack([torch.roll(x[:S], shifts=(2 * f, f), dims=(1, 2)) for f in range(F)], 1).contiguous()
    plain = {k: v.clone() for k, v in air.track(frames).items()}
    t0 = air.tracker(S, F)
    out = air.track(frames, temporal=1)
    t1 = air.tracker(S, F, temporal=1)
    assert t1 is not t0 and isinstance(t1.provider, TemporalProposer) and not isinstance(t0.provider, TemporalProposer)
    assert (t1.provider.proposals, t1.provider.rounds) == (1, 1) and air.tracker(S, F) is t0 and air.tracker(S, F, temporal=(1, 1)) is t1
    assert tuple(out["cand_state"].shape) == (1, S * F, 6) and tuple(out["track_id"].shape) == (3, S * F)
    assert (out["objective"] >= out["objective_start"]).all() and (out["num_objects"] <= 3).all()
    assert torch.equal(out["num_objects_start"], plain["num_objects"])      # the start parse is the plain stack's parse
    gt = torch.zeros(S, F, 2, 4)
    gt[..., 2:] = 10.0
    scores, t2 = air.score_track(frames, gt, temporal=(1, 2), gt_instances=torch.full((S, F, 50, 50), -1, dtype=torch.int8))
    assert t2 is not t1 and t2.provider.rounds == 2 and tuple(air.tracked["cand_state"].shape) == (2, S * F, 6)
    assert int(scores["seq_counts"][:, 0].sum()) == S * F * 2 and air.track_scorer.parser is t2.provider
    tp = air.temporal_proposer(S, F, proposals=1, rounds=1)
    assert isinstance(tp, TemporalProposer) and air.temporal_proposer(S, F) is tp
    tp.load_from(air._engine)
    rep = tp.parse(frames.reshape(S * F, 50, 50))
    tp.synchronize()
    for k in ("kept_step", "objective", "cand_state", "what", "owner"):      # the same repair as behind the tracker, without identities
        assert same_bits(rep[k], out[k]), k
    assert tuple(rep["partner"].shape) == (1, 1, S * F) and "track_id" not in rep
    for bad in (0, (1, 0), (4, 1), "x", True):
        with pytest.raises(ValueError):
            air.track(frames, temporal=bad)
    with pytest.raises(ValueError, match="ParticleParser"):
        TemporalProposer(types.SimpleNamespace(KIND="particle", engine=air._engine, R=S * F, T=3), F)
    with pytest.raises(ValueError, match="TiledSceneParser"):
        TemporalProposer(air.tiled_parser(1, (75, 75)), 1)


def test_training_script_track_temporal_option(gpu_device, tmp_path, capsys):
    import json
    import os
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--track-eval", "4:2.5",
                            "--track-temporal", "1,2"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_track_score"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count(" track score ") == 2
    for l in rec:
        assert l["n_frames"] == 4 and l["frames"] == 64 and 0 <= l["temporal_kept"] <= 64 * 3
    stack = next(iter(air._trackers.values()))
    assert isinstance(stack[-2], temporal.TemporalProposer) and (stack[-2].proposals, stack[-2].rounds, stack[-2].F) == (1, 2, 4)
    assert tuple(air.tracked["cand_state"].shape) == (2, 64, 6)
    for bad in (["--track-temporal", "1"], ["--track-eval", "4", "--track-temporal", "0"], ["--track-eval", "4", "--track-temporal", "1,2,3"],
                ["--track-eval", "4", "--track-temporal", "many"]):
        with pytest.raises(SystemExit):
            multi_mnist.main(bad)
