"""GPU tests of scene parsing (attend_infer_repeat_amd/parse.py, csrc/parse_kernels.hip): the count rule, the boxes and the object
table of air_parse_objects against float64 / the source rows, air_parse_render against the engine's own canvas (bit for bit), the
float64 inverse warp and the float64 arg-max, SceneParser end to end against the float64 oracle at the mode (noise 0 / 0 / -1),
graph replay against eager, the training engine left untouched, and the public surface.

Bars.  count_prob and score are a float64 quotient rounded to fp32 (and up to T fp32 adds of numbers <= 1): 1e-6 (|ref| + 1).  A box
coordinate is a handful of fp32 roundings of terms of size max(W, H) (1 + |s| + |t|): 1e-6 of that.  Everything that comes out of the
decoder + canvas arithmetic uses the engine suite's per-sample output bars OUT_TOL = 1e-4 (worst element / tensor max) and
OUT_L2 = 3e-5 (relative L2); the bf16 case the 2e-3 of test_engine.py::test_bf16_mfma_path_matches_bf16_emulating_oracle.  The owner
map is compared where those bars can settle the decision: a pixel is skipped when its top layer value is within
m = OUT_TOL * max|layer| of the threshold, or of the runner-up; at most 0.5 % of the pixels may be skipped."""
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import air_oracle as O
from test_engine import CONFIGS, OUT_L2, OUT_TOL, check_tensor, f64, make_pair

pytestmark = pytest.mark.gpu

MASK_THRESHOLD = 0.02
C4_B6 = (O.AIRConfig(img_size=(100, 100), crop_size=(28, 28), max_steps=5), 6)      # BASELINE configs[3] shapes: several row bands


def engine_config(ocfg, mfma_dtype="f32", **kw):
    from attend_infer_repeat_amd.engine_config import EngineConfig
    fields = {f.name for f in dataclasses.fields(EngineConfig)}
    d = {k: v for k, v in dataclasses.asdict(ocfg).items() if k in fields}
    d.update(kw)
    return EngineConfig(mfma_dtype=mfma_dtype, **d)


SENTINEL_F, SENTINEL_I = -777.0, -7


def run_objects(prob, n_in, where, what, H, W):
    """air_parse_objects alone on device tensors (current stream); every output starts as a sentinel fill"""
    from attend_infer_repeat_amd import _lib, hip as Hh
    T, R, A = what.shape
    dev = what.device
    ff = lambda *s: torch.full(s, SENTINEL_F, device=dev)
    fi = lambda *s: torch.full(s, SENTINEL_I, dtype=torch.int32, device=dev)
    out = dict(num_objects=fi(R), count_prob=ff(R), presence=ff(T, R), score=ff(T, R), boxes=ff(T, R, 4), offsets=fi(R + 1),
               obj_image=fi(T * R), obj_step=fi(T * R), obj_box=ff(T * R, 4), obj_score=ff(T * R), obj_where=ff(T * R, 4),
               obj_what=ff(T * R, A))
    p = Hh._p
    st = Hh.lib().air_parse_objects(p(prob), p(n_in), p(where), p(what), T, R, A, H, W, p(out["num_objects"]), p(out["count_prob"]),
                                    p(out["presence"]), p(out["score"]), p(out["boxes"]), p(out["offsets"]), p(out["obj_image"]),
                                    p(out["obj_step"]), p(out["obj_box"]), p(out["obj_score"]), p(out["obj_where"]),
                                    p(out["obj_what"]), Hh._stream())
    _lib.check(st, "air_parse_objects")
    torch.cuda.synchronize()
    return out


def run_render(glimpse, where, presence, obs, mult, std, img, crop, layers=True, thr=MASK_THRESHOLD):
    """air_parse_render alone (current stream), banded as the engine bands its canvas; rec = the band shares added in band order"""
    from attend_infer_repeat_amd import _lib, hip as Hh
    T, R = presence.shape
    (H, W), (h, w) = img, crop
    dev = presence.device
    L, p = Hh.lib(), Hh._p
    nb = int(L.air_canvas_unroll_bands(R, H))
    out = dict(reconstruction=torch.full((R, H, W), SENTINEL_F, device=dev), rec_parts=torch.full((nb, R), SENTINEL_F, device=dev),
               owner=torch.full((R, H, W), 99, dtype=torch.int8, device=dev),
               area=torch.full((T, R), SENTINEL_I, dtype=torch.int32, device=dev),        # (the entry zeroes it itself)
               layers=torch.full((T, R, H, W), SENTINEL_F, device=dev) if layers else None)
    st = L.air_parse_render(p(glimpse), p(where), p(presence), p(obs), float(mult), float(std), float(thr), T, R, H, W, h, w, nb,
                            p(out["reconstruction"]), p(out["rec_parts"]), p(out["owner"]), p(out["area"]), p(out["layers"]),
                            Hh._stream())
    _lib.check(st, "air_parse_render")
    torch.cuda.synchronize()
    rec = out["rec_parts"][0].clone()
    for q in range(1, nb):
        rec = rec + out["rec_parts"][q]
    out["rec"], out["n_bands"] = rec, nb
    return out


# ---- 1. the count rule ---------------------------------------------------------------------------------------------------------
def f64_posterior(p):
    """m_n in float64, in index order; (m, q, n^ = the smallest n attaining the maximum, score_t = sum_{n>t} q_n)"""
    T = len(p)
    m, cum = [], 1.0
    for n in range(T):
        m.append((1.0 - p[n]) * cum)
        cum *= p[n]
    m.append(cum)
    S = 0.0
    for v in m:
        S += v
    q = [v / S for v in m]
    n_hat = max(range(T + 1), key=lambda n: (m[n], -n))
    return m, q, n_hat, [sum(q[t + 1:]) for t in range(T)]


def crafted_rows(T, n_random, seed):
    rows = []
    for n in range(T + 1):                                         # a row whose mode is n
        rows.append([0.9] * n + ([0.1] if n < T else []) + [0.5] * max(T - n - 1, 0))
    rows.append(([0.5, 0.0] + [0.3] * T)[:T])                      # the exact tie m_0 = m_1 = 0.5: the smaller count wins
    rows.append([0.0] * T)
    rows.append([1.0] * T)
    rng = np.random.default_rng(seed)
    while len(rows) < T + 4 + n_random:
        p = [float(np.float32(v)) for v in rng.random(T)]
        top = sorted(f64_posterior(p)[0])[-2:]
        if top[1] - top[0] < 1e-12:                                # a decision float64 itself cannot settle: redrawn
            continue
        rows.append(p)
    return [[float(np.float32(v)) for v in r] for r in rows]


@pytest.mark.parametrize("T,R", [(3, 7), (5, 6), (1, 5)])
def test_count_rule_matches_f64(gpu_device, T, R):
    A, H, W = 5, 28, 36
    n_rows = -(-(T + 4 + 6) // R) * R                             # whole calls of R rows: the crafted ones + random fill
    rows = crafted_rows(T, n_rows - (T + 4), seed=T)
    g = torch.Generator().manual_seed(T)
    seen = []
    for lo in range(0, n_rows, R):
        chunk = rows[lo:lo + R]
        prob = torch.tensor(chunk, dtype=torch.float32).t().contiguous().cuda()          # [T, R]
        where, what = torch.randn(T, R, 4, generator=g).cuda(), torch.randn(T, R, A, generator=g).cuda()
        got = run_objects(prob, None, where, what, H, W)
        ref = [f64_posterior(r) for r in chunk]
        n_ref = torch.tensor([r[2] for r in ref])
        assert torch.equal(got["num_objects"].cpu().long(), n_ref), (chunk, got["num_objects"], n_ref)
        assert torch.equal(got["presence"].cpu(), (torch.arange(T)[:, None] < n_ref[None, :]).float())
        cp_ref = torch.tensor([r[1][r[2]] for r in ref], dtype=torch.float64)
        sc_ref = torch.tensor([r[3] for r in ref], dtype=torch.float64).t()
        for name, a, b in (("count_prob", got["count_prob"], cp_ref), ("score", got["score"], sc_ref)):
            err = ((a.cpu().double() - b).abs() / (b.abs() + 1.0)).max().item()
            print("%s: worst |got - ref| / (|ref| + 1) = %.3e" % (name, err))
            assert err <= 1e-6, (name, err)
        seen += n_ref.tolist()
    assert sorted(set(seen)) == list(range(T + 1)), seen           # every count 0..T occurred
    assert f64_posterior(rows[T + 1])[2] == 0 and f64_posterior(rows[T + 1])[0][:2] == [0.5, 0.5]        # the tie row is a tie


def test_given_counts_are_clipped_and_need_no_probabilities(gpu_device):
    T, R, A = 3, 7, 5
    g = torch.Generator().manual_seed(3)
    where, what = torch.randn(T, R, 4, generator=g).cuda(), torch.randn(T, R, A, generator=g).cuda()
    prob = torch.rand(T, R, generator=g).cuda()
    n_in = torch.tensor([-2, T + 6, 0, 1, 2, 3, 1], dtype=torch.int32).cuda()
    want = torch.tensor([0, T, 0, 1, 2, 3, 1])
    for pr in (prob, None):                                        # presence_prob = NULL is accepted with given counts
        got = run_objects(pr, n_in, where, what, 28, 36)
        assert torch.equal(got["num_objects"].cpu().long(), want)
        assert torch.equal(got["presence"].cpu(), (torch.arange(T)[:, None] < want[None, :]).float())
        assert got["offsets"].tolist() == [0] + torch.cumsum(want, 0).tolist()
    assert torch.isnan(got["count_prob"]).all() and torch.isnan(got["score"]).all()        # no posterior was given
    # with the probabilities the scores are the model's, whatever count was given
    got = run_objects(prob, n_in, where, what, 28, 36)
    ref = [f64_posterior([float(v) for v in prob[:, r].tolist()]) for r in range(R)]
    cp_ref = torch.tensor([ref[r][1][int(want[r])] for r in range(R)], dtype=torch.float64)
    assert ((got["count_prob"].cpu().double() - cp_ref).abs() <= 1e-6 * (cp_ref.abs() + 1)).all()


# ---- 2. boxes ------------------------------------------------------------------------------------------------------------------
def test_boxes_match_f64_attention_box(gpu_device):
    from attend_infer_repeat_amd.evaluation import attention_box
    T, R, A, H, W = 3, 7, 5, 28, 36
    g = torch.Generator().manual_seed(5)
    where = torch.randn(T, R, 4, generator=g)
    where[0, 0] = torch.tensor([-0.75, 0.3, 0.4, -0.2])            # a negative sx
    where[1, 2] = torch.tensor([1e-3, 0.9, -1e-3, -0.9])           # a row as guard_eps = 1e-3 leaves it (|s| floored, sign kept)
    where[2, 6] = torch.tensor([1.0, 0.0, 1.0, 0.0])               # the whole canvas
    where = where.cuda()
    got = run_objects(None, torch.zeros(R, dtype=torch.int32).cuda(), where, torch.zeros(T, R, A).cuda(), H, W)
    wh = where.cpu()
    assert got["boxes"][2, 6].tolist() == [0.0, 0.0, float(W), float(H)]
    worst = 0.0
    for t in range(T):
        for r in range(R):
            sx, tx, sy, ty = (float(v) for v in wh[t, r])
            ref = attention_box([sx, tx, sy, ty], W, H)            # float64 on the device's own fp32 `where`
            for k, (s, tt) in enumerate(((sx, tx), (sy, ty), (sx, tx), (sy, ty))):
                bound = 1e-6 * max(W, H) * (1 + abs(s) + abs(tt))
                err = abs(float(got["boxes"][t, r, k]) - ref[k])
                worst = max(worst, err / bound)
                assert err <= bound, (t, r, k, err, bound)
    print("boxes: worst error / bound = %.3f" % worst)


# ---- 3. object table -----------------------------------------------------------------------------------------------------------
def _check_table(got, n, where, what):
    T, R, A = what.shape
    n = n.cpu().long()
    offs = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(n, 0)])
    assert torch.equal(got["offsets"].cpu().long(), offs)
    total = int(offs[-1])
    mask = (torch.arange(T)[None, :] < n[:, None])                 # [R, T]: image-major, step order inside an image
    r_idx, t_idx = mask.nonzero(as_tuple=True)
    assert torch.equal(got["obj_image"][:total].cpu().long(), r_idx) and torch.equal(got["obj_step"][:total].cpu().long(), t_idx)
    pick = lambda x: x.cpu()[t_idx, r_idx]
    assert torch.equal(got["obj_box"][:total].cpu(), pick(got["boxes"]))
    assert torch.equal(got["obj_score"][:total].cpu(), pick(got["score"]))
    assert torch.equal(got["obj_where"][:total].cpu(), pick(where)) and torch.equal(got["obj_what"][:total].cpu(), pick(what))
    # rows at and beyond offsets[R] are not written
    for k in ("obj_box", "obj_score", "obj_where", "obj_what"):
        assert (got[k][total:] == SENTINEL_F).all(), k
    for k in ("obj_image", "obj_step"):
        assert (got[k][total:] == SENTINEL_I).all(), k


@pytest.mark.parametrize("A", [5, 12])                             # A % 4 != 0: the 4-byte path; 12: 16-byte vectors
@pytest.mark.parametrize("R", [1, 7, 300, 5000])
def test_object_table_is_the_source_rows(gpu_device, R, A):
    T = 3
    g = torch.Generator().manual_seed(R + A)
    where, what = torch.randn(T, R, 4, generator=g).cuda(), torch.randn(T, R, A, generator=g).cuda()
    prob = torch.rand(T, R, generator=g).cuda()
    n = (torch.arange(R) % (T + 1)).to(torch.int32).cuda()
    _check_table(run_objects(prob, n, where, what, 50, 50), n, where, what)
    if R == 300:
        for fill in (0, T):                                        # an empty table, a full one
            n = torch.full((R,), fill, dtype=torch.int32).cuda()
            got = run_objects(prob, n, where, what, 50, 50)
            _check_table(got, n, where, what)
            assert int(got["offsets"][-1]) == fill * R


# ---- 4. render, kernel alone ---------------------------------------------------------------------------------------------------
RENDER_CASES = {"tiny": CONFIGS["tiny"], "t1_b5": CONFIGS["t1_b5"], "rect_t5": CONFIGS["rect_t5"], "mnist_b8": CONFIGS["mnist_b8"],
                "c4_b6": C4_B6}


def mode_forward(ocfg, B):
    """zero-noise forward of make_pair's engine: (engine, raw glimpses [T, B, h, w], where [T, B, 4])"""
    eng, params, obs, _ = make_pair(ocfg, B, seed=1, bias_std=0.1)
    eng.set_noise(torch.zeros_like(eng.eps_where), torch.zeros_like(eng.eps_what), torch.full_like(eng.u_pres, -1.0))
    eng.forward(sample_noise=False)
    eng.synchronize()
    return eng, params, obs, eng.gd.out[-1].view(eng.T, B, *ocfg.crop_size), eng.where


def f64_layers(glimpse, where, img, mult):
    T, B = glimpse.shape[:2]
    g, w = glimpse.double().cpu(), where.double().cpu()
    return torch.stack([O.st_write(g[t], w[t], img) for t in range(T)], 0) * mult                   # [T, B, H, W]


def check_owner(owner, layers_ref, n, thr):
    """the device's owner map against the float64 arg-max where OUT_TOL can settle the decision; returns the skipped share"""
    T, B = layers_ref.shape[:2]
    present = (torch.arange(T)[:, None] < n.cpu().long()[None, :])[:, :, None, None]
    vals = torch.where(present, layers_ref, torch.full_like(layers_ref, -float("inf")))
    top, arg = vals.max(0)                                         # (the first maximal index: the smallest step)
    second = vals.scatter(0, arg[None], -float("inf")).max(0).values
    m = OUT_TOL * layers_ref.abs().max().item()
    ref = torch.where(top > thr, arg, torch.full_like(arg, -1))
    skip = ((top - thr).abs() <= m) | ((top > thr) & (top - second <= m))
    ref = torch.where((n.cpu().long() == 0)[:, None, None], torch.full_like(ref, -1), ref)
    skip = skip & (n.cpu().long() > 0)[:, None, None]
    bad = (owner.cpu().long() != ref) & ~skip
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:5])
    return skip.double().mean().item()


@pytest.mark.parametrize("name", list(RENDER_CASES))
def test_render_matches_canvas_kernel_f64_warp_and_f64_argmax(gpu_device, name):
    from attend_infer_repeat_amd import _lib, hip as Hh
    ocfg, B = RENDER_CASES[name]
    eng, params, obs, glimpse, where = mode_forward(ocfg, B)
    T, (H, W), (h, w) = eng.T, ocfg.img_size, ocfg.crop_size
    mult, std = float(ocfg.output_multiplier), float(ocfg.output_std)
    n = (torch.arange(B) % (T + 1)).to(torch.int32).cuda()
    presence = run_objects(None, n, where, eng.what, H, W)["presence"]
    got = run_render(glimpse, where, presence, eng.obs, mult, std, (H, W), (h, w))
    # the engine's own canvas entry with the same presences on the same buffers: the same bits
    canvas, rec_ref = torch.zeros(B, H * W).cuda(), torch.zeros(B).cuda()
    p = Hh._p
    _lib.check(Hh.lib().air_canvas_unroll_fwd(p(glimpse), p(where), p(presence), p(eng.obs), None, p(canvas), p(rec_ref), T, B, H, W,
                                              h, w, mult, std, Hh._stream()), "air_canvas_unroll_fwd")
    torch.cuda.synchronize()
    assert torch.equal(got["reconstruction"].reshape(B, -1), mult * canvas)
    check_tensor("parse_render", name, "out", "rec", got["rec"], rec_ref, OUT_TOL, OUT_L2)
    # layers against the float64 inverse warp; exactly zero for absent steps
    ref = f64_layers(glimpse, where, (H, W), mult)
    absent = (torch.arange(T)[:, None] >= n.cpu().long()[None, :])
    assert (got["layers"].cpu()[absent] == 0).all()
    ref_present = torch.where(absent[:, :, None, None], torch.zeros_like(ref), ref)
    check_tensor("parse_render", name, "out", "layers", got["layers"], ref_present, OUT_TOL, OUT_L2)
    # owner against the float64 arg-max, area = the histogram of the device's own owner map
    skipped = check_owner(got["owner"], ref, n, MASK_THRESHOLD)
    print("%s: %d bands, skipped share of the owner map %.4f %%" % (name, got["n_bands"], 100 * skipped))
    assert skipped <= 0.005, skipped
    own = got["owner"].cpu().long()
    hist = torch.stack([(own == t).reshape(B, -1).sum(1) for t in range(T)], 0)
    assert torch.equal(got["area"].cpu().long(), hist)
    assert (own >= -1).all() and (own < n.cpu().long()[:, None, None]).all()
    owned_steps = (hist.sum(1) > 0).tolist()
    print("%s: steps that own pixels somewhere in the batch: %s" % (name, owned_steps))
    assert any(owned_steps) or T == 1                              # the arg-max check is not vacuous
    # an image without objects: all-zero reconstruction, no owner, zero areas
    empty = (n.cpu() == 0)
    assert (got["reconstruction"].cpu()[empty] == 0).all() and (own[empty] == -1).all() and (got["area"].cpu()[:, empty] == 0).all()
    # without the optional outputs the others are the same bits
    lean = run_render(glimpse, where, presence, eng.obs, mult, std, (H, W), (h, w), layers=False)
    for k in ("reconstruction", "rec", "owner", "area"):
        assert torch.equal(lean[k], got[k]), k


# ---- 5. end to end against the float64 oracle ----------------------------------------------------------------------------------
def mode_noise(ocfg, B):
    T = ocfg.max_steps
    return {"eps_where": torch.zeros(T, B, 4), "eps_what": torch.zeros(T, B, ocfg.n_appearance), "u_pres": -torch.ones(T, B, 1)}


def make_parser(ocfg, B, params, mfma_dtype="f32", **kw):
    from attend_infer_repeat_amd.parse import SceneParser
    ps = SceneParser(engine_config(ocfg, mfma_dtype), B, seed=1, mask_threshold=MASK_THRESHOLD, **kw)
    ps.load_parameters(params)
    ps.set_global_step(20000)
    return ps


def e2e_case(name):
    ocfg, B = CONFIGS[name]
    if name == "rect_t5":                                          # confident count heads: both 0 and 5 occur
        ocfg = dataclasses.replace(ocfg, step_bias=2.0)
    params = O.init_params(ocfg, seed=1, bias_std=0.1)
    if name == "rect_t5":
        last = "steps/%d/w" % len(ocfg.steps_pred_hidden)
        params[last] = params[last] * 30
    obs, _ = O.synthetic_batch(ocfg, B, seed=11)
    return ocfg, B, params, obs


def _check_parse_against_oracle(name, ocfg, B, params, obs, mfma_dtype, tol, tol_l2):
    res = O.unroll(f64(params), ocfg, obs.double(), f64(mode_noise(ocfg, B)))
    T, (H, W) = ocfg.max_steps, ocfg.img_size
    assert (res["presence"] == 1).all()                            # nothing is masked upstream
    ps = make_parser(ocfg, B, params, mfma_dtype, keep_layers=True)
    out = ps.parse(obs.cuda())
    ps.synchronize()
    for k in ("what", "where", "presence_prob"):
        check_tensor("parse_e2e", name, "out", k, out[k].reshape(res[k].shape), res[k], tol, tol_l2)
    q_ref = O.bernoulli_to_modified_geometric(res["presence_prob"].reshape(T, B).t())
    check_tensor("parse_e2e", name, "out", "q_n", out["num_steps_posterior"], q_ref, tol, tol_l2)
    top2 = q_ref.double().sort(1, descending=True).values[:, :2]
    gap = top2[:, 0] - top2[:, 1]
    n_ref = q_ref.double().argmax(1)
    checked = gap > 1e-3
    n_got = out["num_objects"].cpu().long()
    print("%s: counts %s (oracle %s), smallest top-two gap %.2e, %d of %d images checked"
          % (name, n_got.tolist(), n_ref.tolist(), gap.min().item(), int(checked.sum()), B))
    assert checked.double().mean().item() >= 0.75
    assert torch.equal(n_got[checked], n_ref[checked])
    # the reconstruction with the oracle's presence mask (on the images whose count is settled)
    same = checked & (n_got == n_ref)
    layers = torch.stack([O.st_write(res["glimpse_raw"][t].reshape(B, *ocfg.crop_size), res["where"][t], (H, W)) for t in range(T)], 0)
    mask = (torch.arange(T)[:, None] < n_ref[None, :]).double()[:, :, None, None]
    rec_ref = ocfg.output_multiplier * (mask * layers).sum(0)
    if same.any() and rec_ref[same].abs().max() > 0:
        check_tensor("parse_e2e", name, "out", "reconstruction", out["reconstruction"].cpu()[same], rec_ref[same], tol, tol_l2)
    z = (obs.double() - rec_ref) / ocfg.output_std
    rec_term = (0.5 * z * z + 0.5 * math.log(2 * math.pi) + math.log(ocfg.output_std)).reshape(B, -1).sum(1)
    check_tensor("parse_e2e", name, "out", "rec", out["rec"].cpu()[same], rec_term[same], tol, tol_l2)
    # the same with given counts r mod (T + 1): every count renders, whatever the model's own mode is (the latents do not move)
    n_giv = torch.arange(B) % (T + 1)
    out_g = ps.parse(obs.cuda(), n_giv.to(torch.int32).cuda())
    ps.synchronize()
    assert torch.equal(out_g["num_objects"].cpu().long(), n_giv)
    mask_g = (torch.arange(T)[:, None] < n_giv[None, :]).double()[:, :, None, None]
    rec_g = ocfg.output_multiplier * (mask_g * layers).sum(0)
    check_tensor("parse_e2e", name, "out", "reconstruction_given", out_g["reconstruction"], rec_g, tol, tol_l2)
    check_tensor("parse_e2e", name, "out", "layers_given", out_g["layers"], ocfg.output_multiplier * mask_g * layers, tol, tol_l2)
    out = ps.parse(obs.cuda())
    ps.synchronize()
    # the read-outs agree with each other
    assert torch.equal(out["presence"].cpu(), (torch.arange(T)[:, None] < n_got[None, :]).float())
    assert (out["count_prob"].cpu() - out["num_steps_posterior"].cpu()[torch.arange(B), n_got]).abs().max() <= 1e-6
    assert int(out["offsets"][-1]) == int(n_got.sum())
    return n_got


@pytest.mark.parametrize("name", ["mnist_b8", "rect_t5", "tiny"])
def test_parse_matches_f64_oracle_at_the_mode(gpu_device, name):
    ocfg, B, params, obs = e2e_case(name)
    n_got = _check_parse_against_oracle(name, ocfg, B, params, obs, "f32", OUT_TOL, OUT_L2)
    if name == "rect_t5":
        assert {0, 5} <= set(n_got.tolist()), n_got


def test_bf16_parse_matches_bf16_emulating_oracle(gpu_device):
    ocfg, B, params, obs = e2e_case("mnist_b8")
    with O.matmul_mode("bf16"):
        _check_parse_against_oracle("mnist_b8_bf16", ocfg, B, params, obs, "bf16", 2e-3, 2e-3)


# ---- 6. graph ------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager(gpu_device):
    ocfg, B, params, _ = e2e_case("mnist_b8")
    eager, graph = make_parser(ocfg, B, params, keep_layers=True), make_parser(ocfg, B, params, keep_layers=True)
    graph.capture()
    batches = [O.synthetic_batch(ocfg, B, seed=s)[0].cuda() for s in (11, 12)]
    given = torch.tensor([0, 1, 2, 3, 3, 2, 1, 0], dtype=torch.int32).cuda()
    kept = []
    for obs in batches:
        for counts in (None, given, 2):
            a, b = eager.parse(obs, counts), graph.parse(obs, counts)
            eager.synchronize(); graph.synchronize()
            assert set(a) == set(b)
            for k in a:
                assert torch.equal(a[k], b[k]), k
            if counts is None:
                kept.append(b["reconstruction"].clone())
            elif counts is given:
                assert torch.equal(b["num_objects"], given)
            else:
                assert b["num_objects"].tolist() == [2] * B
    assert not torch.equal(kept[0], kept[1]) or kept[0].abs().max() == 0
    assert graph.launch_count() == {"forward": len(graph.engine._plan_fwd), "parse_objects": 1, "parse_render": 1, "rec_sum": 1}
    graph.release_graphs()


# ---- 7. the training engine is only read ---------------------------------------------------------------------------------------
def _mnist_air(B=8, **kw):
    from attend_infer_repeat_amd import mnist_model, utils
    from attend_infer_repeat_amd.data import synthetic_multi_mnist
    AD = utils.AttrDict
    imgs, nums = synthetic_multi_mnist(B, (50, 50), 2, seed=0)
    x, y = torch.from_numpy(imgs).cuda(), torch.from_numpy(nums).cuda()
    torch.manual_seed(0)
    air = mnist_model.AIRonMNIST(x, y, max_steps=3, explore_eps=1e-3, steps_pred_hidden=[128, 64], transform_var_bias=.5,
                                 step_bias=.75, output_multiplier=.5)
    nsp = AD(anneal='exp', init=1. - 1e-15, final=1e-7, steps_div=1e4, steps=1e5, hold_init=1e3)
    ts, _ = air.train_step(1e-4, 0., AD(loc=0., scale=1.), AD(loc=0., scale=1.), AD(loc=0., scale=1.), nsp, **kw)
    return air, ts, x, y


def _train_state(eng):
    eng.synchronize()
    return {k: getattr(eng, k).clone() for k in ("flat_params", "flat_ms", "flat_mg", "flat_mom", "step_dev", "rng_state")}


def test_parse_on_the_model_does_not_disturb_training(gpu_device):
    B, T, A = 8, 3, 50
    air, ts, x, y = _mnist_air(B)
    twin, ts_twin, _, _ = _mnist_air(B)
    for _ in range(2):
        ts(); ts_twin()
    before = _train_state(air._engine)
    out = air.parse()
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert air._engine.global_step == 2 and int(air.global_step) == 2
    # the documented keys and shapes
    shapes = {"num_objects": (B,), "count_prob": (B,), "num_steps_posterior": (B, T + 1), "presence_prob": (T, B), "presence": (T, B),
              "score": (T, B), "boxes": (T, B, 4), "what": (T, B, A), "where": (T, B, 4), "glimpse": (T, B, 20, 20),
              "offsets": (B + 1,), "obj_image": (T * B,), "obj_step": (T * B,), "obj_box": (T * B, 4), "obj_score": (T * B,),
              "obj_where": (T * B, 4), "obj_what": (T * B, A), "reconstruction": (B, 50, 50), "rec": (B,), "owner": (B, 50, 50),
              "area": (T, B)}
    assert {k: tuple(v.shape) for k, v in out.items()} == shapes
    assert out["num_objects"].dtype == torch.int32 and out["owner"].dtype == torch.int8 and out["area"].dtype == torch.int32
    assert out is air.parsed and torch.isfinite(out["reconstruction"]).all() and torch.isfinite(out["rec"]).all()
    ps = air._scene_parser
    assert torch.equal(ps.engine.flat_params, air._engine.flat_params) and int(ps.engine.step_dev.item()) == 2
    # deterministic: the same image again gives the same bits
    first = {k: v.clone() for k, v in out.items()}
    again = air.parse(x)
    assert all(torch.equal(first[k], again[k]) for k in ("num_objects", "boxes", "reconstruction", "owner", "area", "obj_what"))
    ts(); ts_twin()
    air._engine.synchronize(); twin._engine.synchronize()
    assert torch.equal(air._engine.flat_params, twin._engine.flat_params)
    assert torch.equal(air._engine.rng_state, twin._engine.rng_state)
    # the logger against a torch recomputation
    from attend_infer_repeat_amd.evaluation import make_parse_logger
    got = make_parse_logger(air, lambda: (x, y), 2, "test")(itr=3)
    assert set(got) == {"map_num_step_acc", "count_prob", "num_objects"}
    o = air.parse(x)
    gt = y.sum(0).reshape(-1).long()
    assert got["map_num_step_acc"] == (o["num_objects"].long() == gt).double().mean().item()
    assert got["num_objects"] == o["num_objects"].double().mean().item()
    assert abs(got["count_prob"] - o["count_prob"].double().mean().item()) <= 1e-12


def test_parse_needs_the_engine(gpu_device):
    from attend_infer_repeat_amd import mnist_model
    from attend_infer_repeat_amd.data import synthetic_multi_mnist
    imgs, nums = synthetic_multi_mnist(4, (50, 50), 2, seed=0)
    air = mnist_model.AIRonMNIST(torch.from_numpy(imgs).cuda(), torch.from_numpy(nums).cuda(), max_steps=3)
    with pytest.raises(NotImplementedError, match="engine"):
        air.parse()
    with pytest.raises(NotImplementedError, match="engine"):
        air.scene_parser()


# ---- 8. surface ----------------------------------------------------------------------------------------------------------------
def test_training_script_parse_eval_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--parse-eval"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_parse"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count(" parse ") == 2
    for l in rec:
        assert 0.0 <= l["map_num_step_acc"] <= 1.0 and 0.0 < l["count_prob"] <= 1.0 and 0.0 <= l["num_objects"] <= 3.0


def test_make_parse_fig(gpu_device, tmp_path):
    pytest.importorskip("matplotlib")
    from attend_infer_repeat_amd.evaluation import make_parse_fig
    air, ts, x, y = _mnist_air(8)
    make_parse_fig(air, str(tmp_path), 7, n_samples=4)
    assert os.path.getsize(os.path.join(tmp_path, "parse_fig_7.png")) > 0
