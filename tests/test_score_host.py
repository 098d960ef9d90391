"""Host-only checks of parse scoring: the generator's annotations, average_precision against a numpy loop, the host refusals of
ParseScorer, the three C-ABI entries in the header and the ctypes table, and their argument checks, which return AIR_E_* before
any launch (safe without a GPU)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from attend_infer_repeat_amd import _lib, build
    build.build()
    return _lib.load()


# ---- annotations ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def templates():
    from attend_infer_repeat_amd.data import procedural_digit_templates
    return procedural_digit_templates(300, seed=3)


SETTINGS = {"50x50_0-2": dict(canvas_size=(50, 50), n_objects=(0, 2)),
            "100x100_0-4": dict(canvas_size=(100, 100), n_objects=(0, 4)),
            "overlap": dict(canvas_size=(50, 50), n_objects=(0, 2), with_overlap=True),
            "crowded_retry": dict(canvas_size=(40, 40), n_objects=(0, 2), max_tries=1)}


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_annotations_describe_the_images_and_change_no_draw(templates, name):
    from attend_infer_repeat_amd.data import create_multi_mnist
    tpl, lab = templates
    kw = dict(SETTINGS[name], n_samples=400, seed=11)
    plain = create_multi_mnist(tpl, lab, **kw)
    same = create_multi_mnist(tpl, lab, return_annotations=False, **kw)
    assert sorted(plain) == sorted(same) == ["imgs", "labels", "nums"]
    ann = create_multi_mnist(tpl, lab, return_annotations=True, **kw)
    assert sorted(ann) == ["boxes", "imgs", "instances", "labels", "nums"]
    for k in ("imgs", "labels", "nums"):
        assert np.array_equal(plain[k], same[k]) and np.array_equal(plain[k], ann[k]) and plain[k].dtype == ann[k].dtype, k
    n, (H, W) = 400, kw["canvas_size"]
    G = max(kw["n_objects"])
    boxes, inst = ann["boxes"], ann["instances"]
    assert boxes.shape == (n, G, 4) and boxes.dtype == np.float32
    assert inst.shape == (n, H, W) and inst.dtype == np.int8
    counts = ann["nums"][:, :, 0].sum(0).astype(int)              # cumulative one-hot -> count
    assert counts.max() == G and counts.min() == 0
    assert np.array_equal(inst >= 0, ann["imgs"] > 0)
    assert inst.min() >= -1
    for i in range(n):
        c = counts[i]
        assert inst[i].max() < c, i                               # (no object: all background, -1 < 0)
        assert int((boxes[i, :, 2] > 0).sum()) == c
        assert not boxes[i, c:].any()
        for j in range(c):
            l, t, w, h = boxes[i, j]
            assert l == int(l) and t == int(t) and 0 <= l and 0 <= t and l + w <= W and t + h <= H and w > 0 and h > 0
            if not kw.get("with_overlap"):
                ys, xs = np.nonzero(inst[i] == j)
                assert ys.size > 0
                assert xs.min() >= l and xs.max() < l + w and ys.min() >= t and ys.max() < t + h


def test_retry_path_is_exercised_and_resets_the_annotations(templates):
    """max_tries=1 on a crowded canvas: the sample is started again; nothing of the abandoned attempt may stay behind"""
    from attend_infer_repeat_amd.data import create_multi_mnist
    tpl, lab = templates

    class Counting(np.random.RandomState):
        choices = 0

        def choice(self, *a, **k):
            Counting.choices += 1
            return super().choice(*a, **k)

    kw = dict(SETTINGS["crowded_retry"], n_samples=200)
    ann = create_multi_mnist(tpl, lab, rng=Counting(5), return_annotations=True, **kw)
    counts = ann["nums"][:, :, 0].sum(0).astype(int)
    assert Counting.choices > int((counts > 0).sum())              # more attempts than samples with objects: retries happened
    assert np.array_equal(ann["instances"] >= 0, ann["imgs"] > 0)
    assert np.array_equal((ann["boxes"][:, :, 2] > 0).sum(1), counts)


def test_procedural_multi_mnist_passes_the_keyword_on():
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    a = procedural_multi_mnist(20, seed=2, n_templates=50)
    b = procedural_multi_mnist(20, seed=2, n_templates=50, return_annotations=True)
    assert sorted(a) == ["imgs", "labels", "nums"] and np.array_equal(a["imgs"], b["imgs"])
    assert b["boxes"].shape == (20, 2, 4) and b["instances"].shape == (20, 50, 50)


# ---- average precision ----------------------------------------------------------------------------------------------------------
def ap_loop(scores, tp, n_gt):
    """all-point interpolated AP, plain loops; ties keep arrival order"""
    if n_gt == 0:
        return float("nan")
    idx = sorted(range(len(scores)), key=lambda i: -scores[i])    # sorted() is stable
    hits, prec, rec = 0, [], []
    for rank, i in enumerate(idx, 1):
        hits += int(tp[i])
        prec.append(hits / rank)
        rec.append(hits / n_gt)
    ap, prev = 0.0, 0.0
    for i in range(len(idx)):
        ap += (rec[i] - prev) * max(prec[i:])
        prev = rec[i]
    return ap


def test_average_precision_against_a_loop():
    import torch
    from attend_infer_repeat_amd.score import average_precision
    rng = np.random.RandomState(0)
    cases = [([0.9, 0.8, 0.7], [1, 1, 1], 3, 1.0),
             ([0.9, 0.8, 0.7], [0, 0, 0], 3, 0.0),
             ([0.9, 0.8], [1, 0], 0, None),
             ([0.5, 0.5, 0.5, 0.5], [0, 1, 1, 0], 2, None),       # tied scores: arrival order decides
             ([0.5, 0.5, 0.5, 0.5], [1, 1, 0, 0], 2, 1.0),
             ([0.5, 0.5, 0.5, 0.5], [0, 0, 1, 1], 2, 0.5)]
    s = np.round(rng.rand(200), 2).astype(np.float32)             # rounded: ties among random scores as well
    cases.append((s.tolist(), (rng.rand(200) < 0.6).astype(int).tolist(), 150, None))
    for scores, tp, n_gt, want in cases:
        got = float(average_precision(torch.tensor(scores, dtype=torch.float32), torch.tensor(tp, dtype=torch.bool), n_gt))
        ref = ap_loop(scores, tp, n_gt)
        if n_gt == 0:
            assert math.isnan(got) and math.isnan(ref)
            continue
        assert abs(got - ref) <= 1e-12, (scores[:4], got, ref)
        if want is not None:
            assert abs(got - want) <= 1e-12
    assert float(average_precision(torch.zeros(0), torch.zeros(0, dtype=torch.bool), 4)) == 0.0


# ---- host refusals --------------------------------------------------------------------------------------------------------------
def test_scorer_refuses_before_any_device_work():
    from attend_infer_repeat_amd.score import ParseScorer, check_arguments
    assert check_arguments(2, (0.5, 0.75)) is None and check_arguments(8, [1.0]) is None
    for g in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="max_gt_objects"):
            ParseScorer(None, g)
    for th, what in (((), "between 1 and 16"), (tuple(0.5 + 0.02 * i for i in range(17)), "between 1 and 16"),
                     ((0.5, 0.5), "strictly increasing"), ((0.6, 0.5), "strictly increasing"), ((0.0, 0.5), r"\(0, 1\]"),
                     ((0.5, 1.01), r"\(0, 1\]"), ((float("nan"),), r"\(0, 1\]")):
        with pytest.raises(ValueError, match=what):
            ParseScorer(None, 2, thresholds=th)
    with pytest.raises(ValueError, match="max_batches"):
        ParseScorer(None, 2, max_batches=0)


# ---- header, ctypes, argument checks ----------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_name_the_three_entries():
    from attend_infer_repeat_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "air_hip.h")).read(), flags=re.S)
    for name in ("air_score_contingency", "air_score_match", "air_score_reduce"):
        m = re.search(r"AIR_ENGINE_API\s+int\s+%s\s*\(([^;]*)\);" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert "score_kernels.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 10 and _lib.ENGINE_ABI_VERSION == 5
    assert re.search(r"#define\s+AIR_ABI_VERSION\s+10\b", src) and re.search(r"#define\s+AIR_ENGINE_ABI_VERSION\s+5\b", src)


def _ptr(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def test_score_entries_report_argument_errors(lib):
    f = (ctypes.c_double * 512)()
    F = _ptr(f)                                                   # one zeroed host buffer stands in for every pointer: nothing is launched
    odd = ctypes.c_void_p(F.value + 4)

    def contingency(T=3, G=2, R=2, H=4, W=4, **over):
        a = dict(owner=F, gt=F, cont=F)
        a.update(over)
        return lib.air_score_contingency(a["owner"], a["gt"], T, G, R, H, W, a["cont"], None)

    MATCH_PTRS = ("cont", "boxes", "num_objects", "gt_boxes", "gt_count", "thresholds", "box_iou", "mask_iou", "match", "ari",
                  "best_overlap", "count_err")

    def match(T=3, G=2, K=2, R=2, **over):
        a = {k: F for k in MATCH_PTRS}
        a.update(over)
        return lib.air_score_match(*[a[k] for k in MATCH_PTRS[:6]], T, G, K, R, *[a[k] for k in MATCH_PTRS[6:]], None)

    REDUCE_PTRS = ("num_objects", "gt_count", "count_err", "ari", "best_overlap", "match", "box_iou", "totals_i", "totals_f")

    def reduce(T=3, G=2, K=2, R=2, accumulate=0, **over):
        a = {k: F for k in REDUCE_PTRS}
        a.update(over)
        return lib.air_score_reduce(*[a[k] for k in REDUCE_PTRS[:7]], T, G, K, R, a["totals_i"], a["totals_f"], accumulate, None)

    for fn, names in ((contingency, ("owner", "gt", "cont")), (match, MATCH_PTRS), (reduce, REDUCE_PTRS)):
        for name in names:
            assert fn(**{name: None}) == E_NULL, (fn.__name__, name)
        assert fn(T=0) == E_SHAPE and fn(T=33) == E_SHAPE
        assert fn(G=0) == E_SHAPE and fn(G=9) == E_SHAPE
        assert fn(R=0) == E_SHAPE and fn(R=-3) == E_SHAPE
        assert fn(T=32, G=8, R=(2 ** 31) // 297 + 1) == E_SHAPE   # R (T+1) (G+1) past int32
    for fn in (match, reduce):
        assert fn(K=0) == E_SHAPE and fn(K=17) == E_SHAPE
    assert contingency(H=0) == E_SHAPE and contingency(W=0) == E_SHAPE and contingency(H=-2) == E_SHAPE
    assert contingency(R=1000, H=2048, W=2048) == E_SHAPE         # R H W past int32
    assert contingency(R=1, H=65536, W=65536) == E_SHAPE
    assert contingency(cont=ctypes.c_void_p(F.value + 2)) == E_ALIGN
    assert match(boxes=odd) == E_ALIGN and match(gt_boxes=odd) == E_ALIGN
    assert reduce(totals_i=odd) == E_ALIGN and reduce(totals_f=odd) == E_ALIGN
    assert lib.air_status_string(E_ALIGN).decode().startswith("AIR_E_ALIGN")
