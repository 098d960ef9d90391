"""Host-side logic of the engine that needs no GPU."""
import pytest


def test_flat_layout_switch_carves_disjoint_aligned_arrays(monkeypatch):
    """AIR_FLAT_LAYOUT (placement probe of round 5): the five flat arrays as one arena, packed or on staggered 2 MiB slots -- disjoint,
    zero-filled, 16-byte aligned (vectorised operand loads), the stagger as asked; unset = one allocation each."""
    import torch
    from attend_infer_repeat_amd.engine import AIREngine
    n = 2629124                                                   # configs[1]'s parameter count
    dev = torch.device("cpu")
    monkeypatch.delenv("AIR_FLAT_LAYOUT", raising=False)
    plain = AIREngine._alloc_flat(5, n, dev)
    assert len(plain) == 5 and all(t.shape == (n,) and t.dtype == torch.float32 for t in plain)
    for mode, stagger in (("packed", None), ("stagger:0", 0), ("stagger:4096", 4096), ("stagger:8448", 8448)):
        monkeypatch.setenv("AIR_FLAT_LAYOUT", mode)
        arrs = AIREngine._alloc_flat(5, n, dev)
        ptr = [t.data_ptr() for t in arrs]
        assert all(t.shape == (n,) and t.dtype == torch.float32 and not t.any() for t in arrs)
        assert all(p % 16 == 0 for p in ptr) and all(b - a >= 4 * n for a, b in zip(ptr, ptr[1:]))
        if stagger is not None:
            assert [p % (2 << 20) for p in ptr] == [k * stagger for k in range(5)]
        arrs[1].fill_(1.0)
        assert not arrs[0].any() and not arrs[2].any()
    monkeypatch.setenv("AIR_FLAT_LAYOUT", "stagger:10")
    with pytest.raises(ValueError):
        AIREngine._alloc_flat(5, n, dev)
    monkeypatch.setenv("AIR_FLAT_LAYOUT", "diagonal")
    with pytest.raises(ValueError):
        AIREngine._alloc_flat(5, n, dev)


def test_gradient_summaries_norm_ratio_histogram():
    """evaluation.py:221-248 on plain tensors: global norm, per-variable mean |g| / (|v| + 1e-8), and the histogram's content."""
    import torch
    from attend_infer_repeat_amd.evaluation import gradient_summaries
    g = {"a/w": torch.tensor([[3.0, -4.0], [0.0, 0.0]]), "b": torch.tensor([1.0, float("nan"), 2.0])}
    v = {"a/w": torch.ones(2, 2), "b": torch.full((3,), 2.0)}
    out = gradient_summaries({"a/w": g["a/w"]}, v, histogram=True, bins=4)
    assert abs(out["grad_norm"] - 5.0) < 1e-12 and abs(out["grad_ratio/a/w"] - 7.0 / 4) < 1e-6
    h = out["grad_hist/a/w"]
    assert sum(h["counts"]) == 4 and len(h["edges"]) == 5 and h["edges"][0] == -4.0 and h["edges"][-1] == 3.0 and h["non_finite"] == 0
    assert h["counts"][0] == 1 and h["counts"][-1] == 1 and h["counts"][2] == 2          # -4 | (0, 0) | 3
    hb = gradient_summaries({"b": g["b"]}, v, norm=False, ratio=False, histogram=True, bins=2)["grad_hist/b"]
    assert hb["non_finite"] == 1 and sum(hb["counts"]) == 2
    assert "grad_hist/a/w" not in gradient_summaries({"a/w": g["a/w"]}, v)               # off by default (JSON lines, not event files)


def test_roctx_ranges_are_opt_in(monkeypatch):
    """AIR_ROCTX=1 wraps every eagerly issued plan entry in a roctx range (launch.run_plan, which engine._run is); off by default, and a
    missing library is not an error."""
    import attend_infer_repeat_amd.engine as E
    import attend_infer_repeat_amd.launch as LA
    monkeypatch.setattr(LA, "_ROCTX", [False, None])
    monkeypatch.delenv("AIR_ROCTX", raising=False)
    assert LA._roctx() is None
    monkeypatch.setattr(LA, "_ROCTX", [False, None])
    monkeypatch.setenv("AIR_ROCTX", "1")
    lib = LA._roctx()
    if lib is not None:                          # (the ROCm image ships libroctx64; nested depth is what push returns)
        d0 = lib.roctxRangePushA(b"00 air_test"); d1 = lib.roctxRangePushA(b"01 air_test")
        assert d1 == d0 + 1
        lib.roctxRangePop(); lib.roctxRangePop()
    calls = []
    eng = E.AIREngine.__new__(E.AIREngine)
    E.AIREngine._run(eng, [(lambda a, sp: calls.append((a, sp)) or 0, (7,), "air_fake")], "S")
    assert calls == [(7, "S")]



# ---- gemm_groups: the grouping policy of the plans, on synthetic descriptors (16-byte aligned addresses) ------------------------------
def _gd(ta, tb, M, N, K, A=0x10000, B=0x20000, C=0x30000, colsum=None, lda=None, ldb=None, ldc=None):
    from attend_infer_repeat_amd import _lib
    lda = lda if lda is not None else (M if ta else K)
    ldb = ldb if ldb is not None else (K if tb else N)
    return _lib.AirGemmDesc(ta, tb, M, N, K, A, lda, B, ldb, C, ldc if ldc is not None else N, None, 0, None, 0, 0.0, colsum, 0,
                            None, None, 0, None)


def _shape(groups):
    return [[(d.ta, d.tb, d.M, d.N, d.K) for d in g] for g in groups]


def test_gemm_groups_launch_rule():
    """chunks of 8; the wide / odd split of the throughput regime only; the long-K split above 1,536 tiles; the split-K single entry"""
    from attend_infer_repeat_amd import gemm_groups as G
    nine = [_gd(0, 0, 64, 256, 200) for _ in range(9)]
    out = G.plan_launch(nine, throughput=False, use16=False)
    assert [k for k, _ in out] == [G.GROUPED, G.GROUPED] and [len(g) for _, g in out] == [8, 1]
    assert [d for _, g in out for d in g] == nine                                      # order kept
    wide, odd = _gd(0, 0, 3072, 256, 256), _gd(0, 0, 3072, 1, 256)
    out = G.plan_launch([odd, wide], throughput=True, use16=False)
    assert _shape(g for _, g in out) == [[(0, 0, 3072, 256, 256)], [(0, 0, 3072, 1, 256)]]     # two groups, the wide one first
    out = G.plan_launch([odd, wide], throughput=False, use16=False)
    assert len(out) == 1 and out[0][0] == G.GROUPED and len(out[0][1]) == 2              # latency regime: one group
    long_k, many = _gd(1, 0, 256, 256, 3072), _gd(0, 1, 3072, 256, 256)                 # 256 + 3,072 = 3,328 tiles
    out = G.plan_launch([many, long_k], throughput=False, use16=False)
    assert _shape(g for _, g in out) == [[(1, 0, 256, 256, 3072)], [(0, 1, 3072, 256, 256)]]   # the long-K one first
    lone = _gd(0, 0, 272, 256, 2500)                                                   # 17 x 16 = 272 tiles, K >= 1024
    assert G.plan_launch([lone], False, False, allow_splitk=True) == [(G.SPLITK, [lone])]
    assert G.plan_launch([lone], False, False) == [(G.GROUPED, [lone])]
    assert G.plan_launch([lone], False, True, allow_splitk=True) == [(G.GROUPED, [lone])]      # the bf16 data path has no such entry
    assert G.wide_ok(lone, G.tiles16(lone))
    assert G.plan_launch([lone], True, False, allow_splitk=True) == [(G.GROUPED, [lone])]      # throughput regime, wide-eligible


def test_gemm_groups_deferred_weight_gradients():
    """the M % 4 row split, the longest-K-first order, pack()'s 24 / 8 rule, the fp32 and bf16 forms"""
    from attend_infer_repeat_amd import gemm_groups as G
    d = _gd(1, 0, 50, 256, 3072, A=0x10000, C=0x30000, colsum=0x40000, lda=50, ldc=256)
    a, b = G.split_rows(d)
    assert (a.M, b.M) == (48, 2) and (a.N, a.K, b.N, b.K) == (256, 3072, 256, 3072)
    assert a.colsum == 0x40000 and not b.colsum                                         # the bias gradient stays with the first part
    assert (a.A, a.C) == (0x10000, 0x30000) and b.A == 0x10000 + 192 and b.C == 0x30000 + 192 * 256
    assert (b.lda, b.ldb, b.ldc, b.B) == (d.lda, d.ldb, d.ldc, d.B)
    same = _gd(1, 0, 12, 256, 3072)
    assert G.split_rows(same) == [same]
    sizes = lambda n_wide, n_odd: [len(g) for g in G.pack(list(range(n_wide + n_odd)), n_wide)]
    assert sizes(11, 8) == [19] and sizes(3, 4) == [3, 4] and sizes(0, 10) == [8, 2] and sizes(30, 3) == [24, 9]
    assert G.pack(list(range(7)), 3) == [[0, 1, 2], [3, 4, 5, 6]]
    probs = [_gd(1, 0, 256, 256, 1024), d, _gd(1, 0, 256, 1, 3072), _gd(1, 0, 128, 256, 4096)]
    fp32 = G.deferred_dw_groups(probs, bf16=False)
    # (longest K first among the wide-eligible; five problems are "8 or fewer": pack() keeps the two kinds apart, as for (3, 4))
    assert _shape(fp32) == [[(1, 0, 128, 256, 4096), (1, 0, 48, 256, 3072), (1, 0, 256, 256, 1024)], [(1, 0, 2, 256, 3072), (1, 0, 256, 1, 3072)]]
    assert [len(g) for g in G.deferred_dw_groups(probs * 3, bf16=False)] == [15]          # fp32: one launch once the mixed form applies
    many = [_gd(1, 0, 64, 64, 1024 + 4 * i) for i in range(10)] + [_gd(1, 0, 3, 64, 512)]
    bf16 = G.deferred_dw_groups(many, bf16=True)
    assert [len(g) for g in bf16] == [8, 2, 1] and [d.K for d in bf16[0]] == [1060 - 4 * i for i in range(8)]


def test_gemm_groups_fold_predicates():
    """what the folded closing update asks of a grouped launch: the wide-tile weight-gradient regime, a short-K streaming problem mixed
    with tile problems, the parameter tensors a launch reads and the head tensors it forms"""
    from attend_infer_repeat_amd import gemm_groups as G
    dw = lambda M, N, K, **kw: _gd(1, 0, M, N, K, **kw)
    assert G.wide_form([dw(2500, 256, 512), dw(256, 256, 512)], 1000) and not G.wide_form([dw(2500, 256, 192)], 1000)
    assert not G.wide_form([dw(2500, 256, 512), _gd(0, 1, 64, 256, 256)], 1000) and not G.wide_form([dw(256, 256, 512)], 1000)
    short, tile = dw(4096, 256, 64), dw(256, 256, 512)
    assert G.shortk_mixed([short, tile], True, 4096) and not G.shortk_mixed([short, short], True, 4096)
    assert not G.shortk_mixed([short, tile], False, 4096) and not G.shortk_mixed([short, tile], True, 8192)
    p0, g0, spans = 0x100000, 0x200000, [(0, 1000), (1000, 1256), (1256, 5000)]
    dx = _gd(0, 1, 64, 256, 256, A=0x500000, B=p0 + 4 * 1256)
    assert G.tensors_read([dx, tile], p0, p0 + 4 * 5000, spans) == [(1256, 5000)]
    w = dw(10, 100, 64, C=g0, colsum=g0 + 4 * 1000, ldc=100)
    assert G.foldable([dx, w], g0, 2000, []) == (2, [(0, 1000), (1000, 1100)])
    assert G.foldable([dx, w], g0, 2000, [(1000, 1256)]) == (0, []) and G.foldable([w], g0, 0, []) == (0, [])
