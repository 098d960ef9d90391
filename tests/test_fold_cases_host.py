"""The cases of tests/test_fold_kernels.py on the CPU: every case builds (its conditions are asserted where its inputs are made,
tests/fold_cases.py and again here), every case lands on the kernel form its name says when held against the host mirror of the
dispatch rules (attend_infer_repeat_amd/gemm_groups.py), every kernel instantiation behind the folded launches is named by at least
one case, and the references agree with independent ones: the host Philox with Random123's published known answers, the Gaussian
head's backward written out by hand with autograd and with central differences, the float64 RMSProp with the oracle's update."""
import fractions
import math

import numpy as np
import pytest
import torch

import fold_cases as FC
from attend_infer_repeat_amd import gemm_groups as G
from oracle import air_oracle as O

WIDE_MIN_TILES = 1000           # gemm_kernels.hip wide_min_tiles()


# ---- the references against each other ------------------------------------------------------------------------------------------
def test_host_philox_reproduces_the_published_known_answers():
    for ctr, key, out in FC.PHILOX_KAT:
        c, stream, seed = ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32, key[0] | key[1] << 32
        assert FC.philox4x32(c, stream, seed) == list(out)
        assert FC.philox4x32_np(np.array([c], dtype=np.uint64), stream, seed)[0].tolist() == list(out)
    # the array form wraps its counter at 2^64 and agrees with the integer form at every counter
    ctrs = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 5 * 2 ** 33 + 4]
    got = FC.philox4x32_np(np.array(ctrs, dtype=np.uint64), 1, FC.FEED_SEED)
    for c, row in zip(ctrs, got):
        assert row.tolist() == FC.philox4x32(c, 1, FC.FEED_SEED)


def test_noise_reference_layout_and_moments():
    z, u = FC.noise_ref(FC.RNG_SEED, FC.RNG_OFFSET, 4097, 4099)
    assert z.shape == (4097,) and u.shape == (4099,) and z.dtype == torch.float64 and u.dtype == torch.float32
    # quad q of the normals sits at counter offset + q, the uniforms follow the ceil(n_normal / 4) normal quads
    r = FC.philox4x32((FC.RNG_OFFSET + 1025 + 2) & (2 ** 64 - 1), 0, FC.RNG_SEED)
    assert u[8:12].tolist() == [float(np.float32(x >> 8) * np.float32(2.0 ** -24)) for x in r]
    assert bool((u >= 0).all()) and bool((u < 1).all()) and bool(torch.isfinite(z).all())
    big, _ = FC.noise_ref(FC.RNG_SEED, FC.RNG_OFFSET, 200_000, 0)
    assert abs(float(big.mean())) < 0.01 and abs(float(big.std()) - 1.0) < 0.01
    # a prefix of a longer draw is the shorter draw
    assert torch.equal(big[:4097], z)


def test_feeder_indices_are_the_multiply_shift_of_the_first_two_words():
    idx = FC.feeder_indices(FC.FEED_SEED, 3, 5, 37, True)
    for b, v in enumerate(idx):
        r = FC.philox4x32(3 * 5 + b, 1, FC.FEED_SEED)
        assert v == math.floor(fractions.Fraction(r[0] << 32 | r[1], 2 ** 64) * 37)            # floor(u * n), u = the 64-bit word / 2^64
    assert FC.feeder_indices(FC.FEED_SEED, 2 ** 33, 5, 37, False) == [(2 ** 33 * 5 + b) % 37 for b in range(5)]
    many = FC.feeder_indices(FC.FEED_SEED, 0, 4000, 37, True)
    counts = np.bincount(many, minlength=37)
    assert counts.min() > 60 and counts.max() < 160                                      # uniform over the items (mean 108)


def test_gaussian_backward_by_hand_autograd_and_central_differences():
    c = FC.gb_case(0)
    M, D = c["M"], c["D"]
    dsample = c["dsample64"].float()
    auto = FC.gauss_dpre64(c["pre"], c["eps"], dsample, c["dkl_row"])
    hand = FC.gauss_dpre_by_hand(c["pre"], c["eps"], dsample, c["dkl_row"])
    assert float((auto - hand).abs().max()) < 1e-12 * (1 + float(auto.abs().max()))

    def objective(p):
        sample, kl, _, _ = FC.gauss_head64(p, c["eps"].double())
        return float((sample * dsample.double()).sum() + FC.f32v(FC.GB_DKL_SCALE) * (c["dkl_row"].double() * kl).sum())
    p0 = c["pre"].double()
    for (m, j) in [(0, 0), (3, D - 1), (M - 1, D), (17, 2 * D - 1)]:
        e = torch.zeros_like(p0); e[m, j] = 1e-5
        fd = (objective(p0 + e) - objective(p0 - e)) / 2e-5
        assert abs(fd - float(hand[m, j])) < 1e-6 * (1 + abs(fd)), (m, j, fd, float(hand[m, j]))
    # the guard: the floored scale passes no gradient to its raw pre-activation
    cg = FC.gb_case(2)
    gp = FC.gauss_dpre64(cg["pre"], cg["eps"], cg["dsample64"].float(), cg["dkl_row"], cg["guard"])
    assert float(gp[0, cg["D"]]) == 0.0 and bool((gp[1:, cg["D"]:] != 0).all())


def test_rmsprop_reference_is_the_oracles_update():
    cfg = O.AIRConfig()
    gen = torch.Generator().manual_seed(4)
    n = 1001
    p = {"a/w": torch.randn(n, generator=gen).double()}; gr = {"a/w": torch.randn(n, generator=gen).double()}
    slots = O.rmsprop_init(p)
    p0 = p["a/w"].clone()
    O.rmsprop_centered_step(p, gr, slots, cfg)
    got = FC.rmsprop64(p0.float(), gr["a/w"].float(), torch.ones(n), torch.zeros(n), torch.zeros(n), cfg.learning_rate, cfg.rms_decay,
                       cfg.rms_momentum, cfg.rms_eps, 1.0)
    # (the reference takes the float32 values of the inputs and of the hyperparameters: agreement to float32 resolution)
    for a, b in zip(got, (p["a/w"], slots["a/w"]["ms"], slots["a/w"]["mg"], slots["a/w"]["mom"])):
        assert float((a - b).abs().max()) < 3e-7 * (1 + float(b.abs().max()))


def test_prior_reference_covers_the_three_phases_of_every_schedule():
    for anneal, init, final, steps, hold, div, gsteps in FC.PRIOR_SCHEDULES:
        tables = [FC.prior_ref(anneal, init, final, steps, hold, div, s, 5) for s in gsteps]
        assert all(bool(torch.isfinite(t).all()) and t.shape == (6,) for t in tables)
        if anneal is None:
            assert torch.equal(tables[0], tables[2])
        else:
            assert gsteps[0] < hold < gsteps[1] < hold + steps < gsteps[2]
            assert torch.equal(tables[0], O.geometric_prior(init, 5)) and torch.equal(tables[2], O.geometric_prior(final, 5))
            assert not torch.equal(tables[1], tables[0]) and not torch.equal(tables[1], tables[2])


# ---- every case builds, with its conditions, and lands on the form its name says --------------------------------------------------
@pytest.mark.parametrize("name,precision", FC.OPT_RUNS)
def test_opt_case_builds_and_lands_on_its_form(name, precision):
    c = FC.opt_case(name, precision)
    assert bool((c["ms"].double() - c["mg"].double() ** 2 + c["eps"] >= 0.1).all())
    regions = sorted(r for r in c["fold_regions"] + c["ranges"] if r[1] > r[0])
    assert all(a[1] <= b[0] for a, b in zip(regions, regions[1:])) and all(r[0] % 4 == 0 for r in regions)
    assert all(r[0] % 4 == 0 and r[1] % 4 == 0 for r in c["ranges"]) and len(c["ranges"]) <= 4 and c["n_model"] % 4 == 0
    if name == "straddle":
        lo, hi = c["fold_regions"][0]
        assert lo < c["n_model"] < hi and len(c["ranges"]) == 4 and c["grad_scale"] == 0.5
        assert len(set(c["lr_elem"][lo:hi].tolist())) == 2
    if name == "tile16":
        assert c["fold_mask"] == 0b01 and [r[1] - r[0] for r in c["ranges"]] == [40, 0]
    descs = FC.opt_descs(c)
    assert not G.wide_form(descs, WIDE_MIN_TILES) and not G.shortk_mixed(descs, True, 4096)
    form = G.latency_form(descs)
    assert form == c["form"], (name, form)
    if name == "tile32":
        assert sum(G.tiles16(d) for d in descs) == 1600 and min(d.K for d in descs) < 256
    if name == "shortk":
        assert [G.shortk_workgroups(d.M) for d in descs] == [257, 384] and (descs[1].M + 15) // 16 == 386 and descs[1].M % 16


@pytest.mark.parametrize("name", sorted(FC.OPT_DECLINED))
def test_declined_opt_case_is_one_the_rules_decline(name):
    c = FC.opt_case(name, FC.F32, True)
    descs = FC.opt_descs(c)
    assert G.wide_form(descs, WIDE_MIN_TILES) == (name == "wide_regime")
    assert G.shortk_mixed(descs, True, 4096) == (name == "shortk_mixed")


@pytest.mark.parametrize("i", range(len(FC.GB_RUNS)))
def test_gauss_bwd_case_builds_and_lands_on_its_form(i):
    c = FC.gb_case(i)
    descs = FC.gb_descs(c)
    assert sum(G.tiles16(d) for d in descs) <= G.GAUSS_FOLD_MAX_TILES
    assert G.latency_form(descs) == c["form"] and len(descs) == (3 if c["others"] else 1)
    d = descs[c["problem"]]
    assert (d.M, d.N, d.K) == (c["M"], c["D"], c["K"]) and c["ld_pre"] == 2 * c["D"] + 4 and c["ld_dpre"] == 2 * c["D"] + 8
    for o in c["others"]:
        if o["kind"] == "nt_delu":
            assert bool((o["aux"].abs() >= 1e-3).all())


def test_declined_gauss_bwd_case_has_more_than_a_thousand_tiles():
    f = FC.GB_DECLINED
    descs = FC.gb_descs(dict(M=f["M"], D=f["D"], K=f["K"], precision=0), extra=f["extra"])
    assert sum(G.tiles16(d) for d in descs) == 1020 > G.GAUSS_FOLD_MAX_TILES


@pytest.mark.parametrize("i", range(len(FC.GG_CASES)))
def test_gather_case_fits_and_runs_on_the_long_k_body(i):
    c = FC.gg_case(i)
    descs = FC.gg_descs(c)
    assert G.gather_fits(descs, 1 << 20, FC.GG_ITEMS, c["B"], 1 << 22, WIDE_MIN_TILES)
    # what air_gemm_grouped runs the same group on: too few tiles for its wide-tile regime, then the long-K split -- the gather's own body
    assert G.on_long_k_body(descs, WIDE_MIN_TILES) and G.latency_form(descs) == (1, 1, 16)
    assert all(0 <= v < FC.GG_N_ITEMS for v in c["idx"]) and torch.equal(c["obs"], c["data"][torch.tensor(c["idx"])])


def test_fits_cases_against_the_mirror():
    fits = lambda descs, bg: G.gather_fits(descs, bg["obs"], bg["item_floats"], bg["B"], bg["dataset"], WIDE_MIN_TILES)
    for name, change in FC.FITS_ACCEPTED.items():
        descs, bg = FC.fits_launch(change)
        assert fits(descs, bg), name
        assert G.on_long_k_body(descs, WIDE_MIN_TILES) and G.latency_form(descs) == (1, 1, 16), name
    for name, change in FC.FITS_DECLINED.items():
        descs, bg = FC.fits_launch(change)
        assert not fits(descs, bg), name
        d = descs[0]
        if name.startswith("off the long-K form"):
            # ... and for no other reason: the rule before this test existed (K >= 512, at most 1024 tiles) took them
            assert d.K >= 512 and G.tiles16(d) <= 1024 and d.K < 8 * min(d.M, d.N) and G.latency_form(descs) == (1, 1, 4)
        if name.endswith("the wide-tile kernels"):
            # ... long K and at most 1024 tiles, which the rule took until it asked for group_long_k alone; air_gemm_grouped looks at
            # the wide-tile regime first, and these groups meet everything it asks there
            assert G.group_long_k(descs) and WIDE_MIN_TILES < G.tiles16(d) <= 1024 and G.wide_ok(d, G.tiles16(d))
    d, bg = FC.fits_launch(FC.FITS_DECLINED["1025 tiles"])
    assert G.tiles16(d[0]) == 1025 and d[0].K >= 8 * min(d[0].M, d[0].N)
    d, bg = FC.fits_launch(FC.FITS_DECLINED["1024 tiles: the wide-tile kernels"])
    assert G.tiles16(d[0]) == 1024
    d, bg = FC.fits_launch(FC.FITS_ACCEPTED["1000 tiles"])
    assert G.tiles16(d[0]) == WIDE_MIN_TILES


def test_gather_edge_shapes_sit_on_both_sides_of_the_wide_tile_regime():
    from attend_infer_repeat_amd import _lib
    both = []
    for B, N, K in (FC.GG_EDGE_TAKEN, FC.GG_EDGE_DECLINED):
        d = _lib.AirGemmDesc(0, 0, B, N, K, 1 << 20, K, 1 << 24, N, 1 << 26, N + 4, None, 0, None, 0, 0.0, None, 0, None, None, 0, None)
        assert G.group_long_k([d]) and B % 16 and K & 15 == 4 and G.wide_ok(d, WIDE_MIN_TILES + 1)     # only the tile count decides
        both.append((G.tiles16(d), G.gather_fits([d], 1 << 20, K, B, 1 << 22, WIDE_MIN_TILES)))
    assert both == [(WIDE_MIN_TILES, True), (WIDE_MIN_TILES + 4, False)]


@pytest.mark.parametrize("i", range(len(FC.GATHER_CASES)))
def test_batch_gather_case_builds(i):
    c = FC.gather_case(i)
    assert len(c["idx"]) == c["B"] and c["data"].shape == (c["n_items"], c["item_floats"])
    if c["n_items"] > 2 ** 20:
        assert max(c["idx"]) >= 2 ** 19                          # the multiply-shift reaches the far half of the items


def _lstm_tiles(M, Hd):
    return ((M + 15) // 16) * ((Hd + 15) // 16)


def _lstm_kernel(M, Hd):
    """the kernel lstm_fwd_launch gives the first step of tests/test_fold_kernels.py: w_h a contiguous [Hd, 4 Hd] tensor and h0 one
    broadcast row (ldh = 0), both at addresses the allocator aligns to 16 bytes"""
    return "lstm_fwd_wide_kernel" if G.lstm_fwd_wide(M, Hd, ldw=4 * Hd, ldh=0) else "lstm_fwd_fused_kernel"


def test_lstm_cases_sit_on_both_sides_of_the_512_tile_edge():
    forms = {}
    for M, Hd in FC.LSTM_PRO_SHAPES:
        forms[(M, Hd)] = _lstm_kernel(M, Hd)
        c = FC.lstm_case(M, Hd)
        _, h, cc, act = FC.lstm_refs(c, FC.F32)
        assert h.shape == (M, Hd) and act.shape == (M, 4 * Hd) and bool(torch.isfinite(act).all())
    assert forms[(1045, 128)] == "lstm_fwd_wide_kernel" and _lstm_tiles(1045, 128) == 528
    assert forms[(64, 256)] == "lstm_fwd_fused_kernel" and _lstm_tiles(64, 256) == 64
    from attend_infer_repeat_amd import _lib

    def gx_form(M, Hd, E, ldx, shifted=False):
        """the body air_gemm_grouped runs the gx product [M, 4Hd, E] on as a launch of its own"""
        d = _lib.AirGemmDesc(0, 0, M, 4 * Hd, E, (1 << 20) + (4 if shifted else 0), ldx, 1 << 22, 4 * Hd, 1 << 24, 4 * Hd + 4, 1 << 26, 1,
                             None, 0, 0.0, None, 0, None, None, 0, None)
        tiles = G.tiles16(d)
        if tiles > WIDE_MIN_TILES and G.wide_ok(d, tiles):
            return "wide"
        return {(1, 1, 4): "tile16", (2, 2, 4): "tile32", (1, 1, 16): "wave16"}[G.latency_form([d])]

    for M, Hd, E, ldx, shifted in FC.FIRST_CASES:
        assert ldx >= E and G.first_step_fits(M, Hd, E)
        c = FC.lstm_case(M, Hd, E, ldx)
        gx, h, cc, act = FC.lstm_refs(c, FC.BF16)
        assert gx.shape == (M, 4 * Hd) and bool(torch.isfinite(h).all())
        # the gx product of the unfused pair runs on the 4-wave 16 x 16 body, whose K order the first step repeats
        assert gx_form(M, Hd, E, ldx, shifted) == "tile16"
    assert max(((M + 15) // 16) * ((4 * Hd + 15) // 16) for M, Hd, *_ in FC.FIRST_CASES) == WIDE_MIN_TILES
    forms = {name: gx_form(*shape) for name, shape in FC.FIRST_DECLINED.items()}
    assert not any(G.first_step_fits(M, Hd, E) for M, Hd, E, _ in FC.FIRST_DECLINED.values())
    assert _lstm_tiles(*FC.FIRST_DECLINED["513 tiles of (M, Hd)"][:2]) == 513 and forms["513 tiles of (M, Hd)"] == "tile16"
    assert forms["1040 tiles of gx: the wide-tile regime"] == "wide" and forms["2048 tiles of gx: 32 x 32 tiles"] == "tile32"
    assert forms["2048 tiles of gx: the wide-tile kernels"] == "wide" and forms["a long K: the 16-wave split"] == "wave16"
    assert all(_lstm_tiles(M, Hd) <= G.FIRST_STEP_MAX_TILES for n, (M, Hd, _, _) in FC.FIRST_DECLINED.items() if not n.startswith("513"))
    # the noise sizes: one beyond the 2048 x 256 quads the noise role's grid holds at once
    assert max((n + 3) // 4 + (u + 3) // 4 for n, u in FC.NOISE_SIZES) > 2048 * 256


@pytest.mark.parametrize("i", range(len(FC.CANVAS_SHAPES)))
def test_canvas_case_builds(i):
    c = FC.canvas_case(i)
    assert c["dpresence64"].shape == (c["T"], c["B"]) and bool((c["presence"] > 0).all()) and bool((c["presence"] < 1).all())
    # d presence by central differences of the float64 objective, at two entries
    tg, tw, obs = c["glimpse"].double(), c["where"].double(), c["obs"].double()

    def objective(p, b):
        """the part of the objective that image b carries (the presence of image b reaches no other)"""
        cv = sum(p[t][b:b + 1, None, None] * O.st_write(tg[t][b:b + 1], tw[t][b:b + 1], (c["H"], c["W"])) for t in range(c["T"]))
        return float((0.5 * ((obs[b:b + 1] - FC.CANVAS_MULT * cv) / FC.CANVAS_STD) ** 2).sum() * FC.f32v(c["loss_scale"]))
    p0 = c["presence"].double()
    for (t, b) in [(0, 0), (c["T"] - 1, c["B"] - 1)]:
        e = torch.zeros_like(p0); e[t, b] = 1e-5
        fd = (objective(p0 + e, b) - objective(p0 - e, b)) / 2e-5
        assert abs(fd - float(c["dpresence64"][t, b])) < 1e-6 * (1 + abs(fd))


# ---- coverage: every kernel instantiation behind the folded launches is named by a case -------------------------------------------
TABLE = ([("gemm_grouped_opt_kernel", form, bf) for form in ((1, 1, 4), (1, 1, 16), (2, 2, 4)) for bf in (False, True)]
         + [("gemm_grouped_opt_sk_kernel",)]
         + [("gemm_grouped_gb_kernel", form, bf) for form in ((1, 1, 4), (1, 1, 16)) for bf in (False, True)]
         + [("gemm_grouped_gather_kernel",), ("batch_gather_kernel",), ("lstm_fwd_first_kernel",), ("step_prologue_body",),
            ("lstm_fwd_fused_kernel",), ("lstm_fwd_wide_kernel",)])


def test_every_kernel_instantiation_of_the_folded_launches_is_reached():
    """the form the mirror gives each case, collected over all cases, against the table of the launches' kernels"""
    reached = set()
    for name, precision in FC.OPT_RUNS:
        form = G.latency_form(FC.opt_descs(FC.opt_case(name, precision)))
        reached.add(("gemm_grouped_opt_sk_kernel",) if form == "shortk" else ("gemm_grouped_opt_kernel", form, bool(precision)))
    for i in range(len(FC.GB_RUNS)):
        c = FC.gb_case(i)
        reached.add(("gemm_grouped_gb_kernel", G.latency_form(FC.gb_descs(c)), bool(c["precision"])))
    if all(G.gather_fits(FC.gg_descs(FC.gg_case(i)), 1 << 20, FC.GG_ITEMS, FC.gg_case(i)["B"], 1 << 22, WIDE_MIN_TILES)
           for i in range(len(FC.GG_CASES))):
        reached.add(("gemm_grouped_gather_kernel",))
    # batch_gather_kernel: both row copies (whole float4s, scalar) and more rows than the 4096 workgroups of its grid
    vec4 = {item_floats % 4 == 0 for item_floats, *_ in FC.GATHER_CASES}
    if vec4 == {True, False} and any(B > 4096 for _, B, *_ in FC.GATHER_CASES):
        reached.add(("batch_gather_kernel",))
    if any(G.first_step_fits(M, Hd, E) for M, Hd, E, *_ in FC.FIRST_CASES):
        reached.add(("lstm_fwd_first_kernel",))
    for M, Hd in FC.LSTM_PRO_SHAPES:
        reached.add((_lstm_kernel(M, Hd),))
    # step_prologue_body: a noise role that draws normals AND uniforms, one that strides (more quads than its 2048 x 256 threads), and a
    # ride on each of the three LSTM kernels (256 and 512 threads)
    quads = [(n + 3) // 4 + (u + 3) // 4 for n, u in FC.NOISE_SIZES]
    rides = {("lstm_fwd_fused_kernel",), ("lstm_fwd_wide_kernel",), ("lstm_fwd_first_kernel",)}
    if (any(n and u for n, u in FC.NOISE_SIZES) and max(quads) > 2048 * 256 and rides <= reached):
        reached.add(("step_prologue_body",))
    missing = [k for k in TABLE if k not in reached]
    assert not missing, f"no case reaches {missing}"
