"""Parse scoring on the device against plain numpy / Python references written here (score.py is never the source of an expected
value): air_score_contingency exactly against np.add.at; air_score_match -- match and count_err exactly, the float64 quotients
rounded to fp32 within 1e-6 (|ref| + 1) (the bar of test_parse.py for such values), ARI also against pair counting over pixels;
air_score_reduce -- integers exactly, float64 sums within 1e-12 of math.fsum, bit-equal reruns; ParseScorer end to end behind a
SceneParser, graph replay, read-only use, and the surface (AIRonMNIST.score_parse, the logger, the training script's option).

Random match cases in which a box IoU lies within 1e-9 of a threshold or of a competing candidate's IoU are redrawn (an fp64
reference cannot decide them); the exact ties are crafted from bit-equal inputs and kept."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-6
THRESHOLDS10 = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))


# ---- references ------------------------------------------------------------------------------------------------------------------
def ref_contingency(owner, gt, T, G):
    R = owner.shape[0]
    cont = np.zeros((R, T + 1, G + 1), np.int32)
    o, g = owner.astype(np.int64).reshape(R, -1), gt.astype(np.int64).reshape(R, -1)
    ok = (o >= -1) & (o <= T - 1) & (g >= -1) & (g <= G - 1)
    rr = np.broadcast_to(np.arange(R)[:, None], o.shape)
    np.add.at(cont, (rr[ok], o[ok] + 1, g[ok] + 1), 1)
    return cont


def ref_box_iou(a, b):
    """a, b: four fp32 numbers (left, top, width, height); float64 in the order the header states"""
    a, b = [float(v) for v in a], [float(v) for v in b]
    if any(math.isnan(v) for v in a + b):
        return 0.0
    ax0, ax1, ay0, ay1 = min(a[0], a[0] + a[2]), max(a[0], a[0] + a[2]), min(a[1], a[1] + a[3]), max(a[1], a[1] + a[3])
    bx0, bx1, by0, by1 = min(b[0], b[0] + b[2]), max(b[0], b[0] + b[2]), min(b[1], b[1] + b[3]), max(b[1], b[1] + b[3])
    iw, ih = max(0.0, min(ax1, bx1) - max(ax0, bx0)), max(0.0, min(ay1, by1) - max(ay0, by0))
    inter = iw * ih
    union = ((ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0)) - inter
    if not (inter > 0 and union > 0):
        return 0.0
    q = inter / union
    return q if math.isfinite(q) else 0.0


def ref_ari(c):
    """c: one image's contingency table [T+1, G+1] (Python integers: exact)"""
    fg = [[int(v) for v in row[1:]] for row in c]
    pairs = lambda n: n * (n - 1) // 2
    N = sum(map(sum, fg))
    if N == 0:
        return float("nan")
    S = sum(pairs(v) for row in fg for v in row)
    P = sum(pairs(sum(row)) for row in fg)
    Q = sum(pairs(sum(col)) for col in zip(*fg))
    C = pairs(N)
    if C == 0:
        return 1.0
    E, M = float(P) * float(Q) / float(C), (float(P) + float(Q)) / 2.0
    return 1.0 if M == E else (S - E) / (M - E)


def ref_ari_pairs(owner, gt):
    """the same index by counting pixel pairs (an independent formulation); owner, gt: flat label arrays of one image"""
    keep = gt >= 0
    p, g = owner[keep].astype(np.int64), gt[keep].astype(np.int64)
    n = p.size
    if n == 0:
        return float("nan")
    iu = np.triu_indices(n, 1)
    same_p, same_g = (p[:, None] == p[None, :])[iu], (g[:, None] == g[None, :])[iu]
    total = same_p.size
    if total == 0:
        return 1.0
    both, in_p, in_g = int((same_p & same_g).sum()), int(same_p.sum()), int(same_g.sum())
    E, M = in_p * in_g / total, (in_p + in_g) / 2.0
    return 1.0 if M == E else (both - E) / (M - E)


def ref_match(cont, boxes, num_objects, gt_boxes, gt_count, thresholds):
    """boxes [T,R,4], gt_boxes [R,G,4] fp32 numpy; thresholds: fp32 values.  Returns float64 / integer numpy arrays."""
    T, R = boxes.shape[:2]
    G, K = gt_boxes.shape[1], len(thresholds)
    out = dict(box_iou=np.zeros((R, T, G)), mask_iou=np.zeros((R, T, G)), match=np.full((K, T, R), -1, np.int8), ari=np.zeros(R),
               best_overlap=np.zeros((R, G)), count_err=np.zeros(R, np.int32))
    for r in range(R):
        nh, g = int(np.clip(num_objects[r], 0, T)), int(np.clip(gt_count[r], 0, G))
        c = cont[r].astype(np.int64)
        for t in range(nh):
            for j in range(g):
                out["box_iou"][r, t, j] = ref_box_iou(boxes[t, r], gt_boxes[r, j])
                n = int(c[t + 1, j + 1])
                union = int(c[t + 1].sum()) + int(c[:, j + 1].sum()) - n
                out["mask_iou"][r, t, j] = n / union if union > 0 else 0.0
        for k, tau in enumerate(thresholds):
            used = set()
            for t in range(nh):
                best, pick = 0.0, -1
                for j in range(g):
                    v = out["box_iou"][r, t, j]
                    if j not in used and v > 0 and v >= float(np.float32(tau)) and v > best:
                        best, pick = v, j
                if pick >= 0:
                    used.add(pick)
                out["match"][k, t, r] = pick
        out["ari"][r] = ref_ari(c)
        for j in range(G):
            out["best_overlap"][r, j] = -1.0 if j >= g else max([out["mask_iou"][r, t, j] for t in range(nh)], default=0.0)
        out["count_err"][r] = nh - g
    return out


def ref_totals(m, num_objects, gt_count, T, G):
    """m: a dict like ref_match's (float arrays are the STORED fp32 values widened).  Returns (integers [6+K], floats [3])."""
    K, _, R = m["match"].shape
    nh, g = np.clip(num_objects, 0, T).astype(int), np.clip(gt_count, 0, G).astype(int)
    fin = np.isfinite(m["ari"])
    ti = [R, int((m["count_err"] == 0).sum()), int(np.abs(m["count_err"].astype(np.int64)).sum()), int(nh.sum()), int(g.sum()),
          int(fin.sum())]
    for k in range(K):
        ti.append(sum(int(m["match"][k, t, r] >= 0) for r in range(R) for t in range(nh[r])))
    tf = [math.fsum(float(v) for v in m["ari"][fin]),
          math.fsum(float(m["best_overlap"][r, j]) for r in range(R) for j in range(g[r])),
          math.fsum(float(m["box_iou"][r, t, m["match"][0, t, r]]) for r in range(R) for t in range(nh[r]) if m["match"][0, t, r] >= 0)]
    return ti, tf


def ap_loop(scores, tp, n_gt):
    if n_gt == 0:
        return float("nan")
    idx = sorted(range(len(scores)), key=lambda i: -scores[i])    # stable: arrival order breaks ties
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


def ref_summary(batches, thresholds, T, G):
    """batches: list of dict(m=ref_match-like dict, num_objects, gt_count, score [T,R]); the figures ParseScorer.summary() names"""
    K = len(thresholds)
    ti, tf = [0] * (6 + K), [[], [], []]
    scores, tps = [], [[] for _ in range(K)]
    for b in batches:
        bi, bf = ref_totals(b["m"], b["num_objects"], b["gt_count"], T, G)
        ti = [x + y for x, y in zip(ti, bi)]
        for i in range(3):
            tf[i].append(bf[i])
        nh = np.clip(b["num_objects"], 0, T)
        for r in range(b["score"].shape[1]):                       # arrival order: batch, image, step
            for t in range(int(nh[r])):
                scores.append(float(b["score"][t, r]))
                for k in range(K):
                    tps[k].append(b["m"]["match"][k, t, r] >= 0)
    tf = [math.fsum(v) for v in tf]
    div = lambda a, b: a / b if b else float("nan")
    images, correct, abs_err, n_pred, n_gt, n_ari = ti[:6]
    out = {"count_acc": div(correct, images), "count_mae": div(abs_err, images)}
    aps = []
    for k, tau in enumerate(thresholds):
        out["precision@%.2f" % tau], out["recall@%.2f" % tau] = div(ti[6 + k], n_pred), div(ti[6 + k], n_gt)
        out["f1@%.2f" % tau] = div(2 * ti[6 + k], n_pred + n_gt)
        aps.append(ap_loop(scores, tps[k], n_gt))
        out["ap@%.2f" % tau] = aps[-1]
    out["map"] = sum(aps) / K
    out.update(fg_ari=div(tf[0], n_ari), mean_best_overlap=div(tf[1], n_gt), matched_box_iou=div(tf[2], ti[6]), images=images,
               objects_pred=n_pred, objects_gt=n_gt)
    return out


def close(got, ref, tol=TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = np.isnan(ref) | (np.abs(got - ref) <= tol * (np.abs(ref) + 1))
    assert ok.all(), (got[~ok][:4], ref[~ok][:4])


def bits_equal(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def same_summary(got, ref):
    assert set(got) == set(ref)
    for k in ref:
        if k in ("images", "objects_pred", "objects_gt"):
            assert got[k] == ref[k], k
        elif math.isnan(ref[k]):
            assert math.isnan(got[k]), k
        else:
            assert abs(got[k] - ref[k]) <= TOL * (abs(ref[k]) + 1), (k, got[k], ref[k])


# ---- launching the entries on their own ----------------------------------------------------------------------------------------------
def run_contingency(owner, gt, T, G, fill=None):
    from attend_infer_repeat_amd import _lib, hip as Hh
    R, H, W = owner.shape
    cont = torch.full((R, T + 1, G + 1), -12345 if fill is None else fill, dtype=torch.int32, device=owner.device)
    _lib.check(Hh.lib().air_score_contingency(Hh._p(owner), Hh._p(gt), T, G, R, H, W, Hh._p(cont), Hh._stream()), "air_score_contingency")
    torch.cuda.synchronize()
    return cont


def run_match(cont, boxes, num_objects, gt_boxes, gt_count, thresholds):
    from attend_infer_repeat_amd import _lib, hip as Hh
    dev = "cuda"
    T, R = boxes.shape[:2]
    G, K = gt_boxes.shape[1], len(thresholds)
    d = dict(cont=torch.as_tensor(cont, dtype=torch.int32, device=dev).contiguous(),
             boxes=torch.as_tensor(boxes, dtype=torch.float32, device=dev).contiguous(),
             num_objects=torch.as_tensor(num_objects, dtype=torch.int32, device=dev),
             gt_boxes=torch.as_tensor(gt_boxes, dtype=torch.float32, device=dev).contiguous(),
             gt_count=torch.as_tensor(gt_count, dtype=torch.int32, device=dev),
             thresholds=torch.tensor(thresholds, dtype=torch.float32, device=dev))
    ff = lambda *s: torch.full(s, -777.0, device=dev)
    out = dict(box_iou=ff(R, T, G), mask_iou=ff(R, T, G), match=torch.full((K, T, R), 77, dtype=torch.int8, device=dev), ari=ff(R),
               best_overlap=ff(R, G), count_err=torch.full((R,), -7, dtype=torch.int32, device=dev))
    p = Hh._p
    st = Hh.lib().air_score_match(p(d["cont"]), p(d["boxes"]), p(d["num_objects"]), p(d["gt_boxes"]), p(d["gt_count"]),
                                  p(d["thresholds"]), T, G, K, R, p(out["box_iou"]), p(out["mask_iou"]), p(out["match"]), p(out["ari"]),
                                  p(out["best_overlap"]), p(out["count_err"]), Hh._stream())
    _lib.check(st, "air_score_match")
    torch.cuda.synchronize()
    return d, out


def run_reduce(d, out, T, G, K, totals_i, totals_f, accumulate):
    from attend_infer_repeat_amd import _lib, hip as Hh
    p = Hh._p
    R = d["num_objects"].numel()
    st = Hh.lib().air_score_reduce(p(d["num_objects"]), p(d["gt_count"]), p(out["count_err"]), p(out["ari"]), p(out["best_overlap"]),
                                   p(out["match"]), p(out["box_iou"]), T, G, K, R, p(totals_i), p(totals_f), int(accumulate),
                                   Hh._stream())
    _lib.check(st, "air_score_reduce")
    torch.cuda.synchronize()


def check_match(out, ref):
    assert torch.equal(out["match"].cpu(), torch.from_numpy(ref["match"]))
    assert torch.equal(out["count_err"].cpu(), torch.from_numpy(ref["count_err"]))
    for k in ("box_iou", "mask_iou", "ari", "best_overlap"):
        close(out[k].cpu().numpy(), ref[k])


# ---- 1. contingency --------------------------------------------------------------------------------------------------------------
def skewed_maps(rng, T, G, R, H, W):
    """labels with skewed probabilities: background dominates, the last labels are rare, one label never occurs (empty bins)"""
    def draw(n_labels):
        p = np.array([8.0] + [1.0 / (1 + i) ** 2 for i in range(n_labels)])
        if n_labels > 1:
            p[1 + n_labels // 2] = 0.0
        return (rng.choice(n_labels + 1, size=(R, H, W), p=p / p.sum()) - 1).astype(np.int8)
    return draw(T), draw(G)


@pytest.mark.parametrize("T,G,R,H,W", [(1, 1, 1, 5, 7), (3, 2, 7, 50, 50), (5, 4, 3, 100, 100), (32, 8, 2, 16, 16)])
def test_contingency_is_exact(gpu_device, T, G, R, H, W):
    rng = np.random.RandomState(T * 100 + G)
    owner, gt = skewed_maps(rng, T, G, R, H, W)
    ref = ref_contingency(owner, gt, T, G)
    assert (T == 1 or (ref == 0).any()) and ref.max() > H * W // 4 and ref.sum() == R * H * W
    o, g = torch.from_numpy(owner).cuda(), torch.from_numpy(gt).cuda()
    for fill in (-12345, 0, 2 ** 30):                              # every bin is written whatever was there
        assert torch.equal(run_contingency(o, g, T, G, fill).cpu(), torch.from_numpy(ref))
    # rows that start at different offsets from a 16-byte boundary (views into larger buffers): the byte path, and a shifted head
    for so, sg in ((3, 3), (1, 6), (0, 9)):
        bo, bg = torch.zeros(R * H * W + 32, dtype=torch.int8).cuda(), torch.zeros(R * H * W + 32, dtype=torch.int8).cuda()
        vo, vg = bo[so:so + R * H * W].view(R, H, W), bg[sg:sg + R * H * W].view(R, H, W)
        vo.copy_(o); vg.copy_(g)
        assert torch.equal(run_contingency(vo, vg, T, G).cpu(), torch.from_numpy(ref)), (so, sg)


def test_contingency_counts_out_of_range_labels_nowhere(gpu_device):
    T, G, R, H, W = 3, 2, 5, 50, 50
    rng = np.random.RandomState(4)
    owner, gt = skewed_maps(rng, T, G, R, H, W)
    clean = ref_contingency(owner, gt, T, G)
    dirty_o, dirty_g = owner.copy(), gt.copy()
    hit_o, hit_g = rng.rand(R, H, W) < 0.03, rng.rand(R, H, W) < 0.03
    hit_o[0] = hit_g[0] = False                                    # image 0 stays clean; image 2 gets the parser's sentinel everywhere
    hit_o[2] = True
    dirty_o[hit_o] = 99
    dirty_g[hit_g] = G
    dirty_o[1, 0, :8] = [T, T + 1, 127, -2, -128, 99, -3, T]
    dirty_g[1, 1, :4] = [G, -2, -128, 127]
    ref = ref_contingency(dirty_o, dirty_g, T, G)
    assert np.array_equal(ref[0], clean[0]) and ref[2].sum() == 0 and 0 < ref[1].sum() < H * W
    got = run_contingency(torch.from_numpy(dirty_o).cuda(), torch.from_numpy(dirty_g).cuda(), T, G).cpu()
    assert torch.equal(got, torch.from_numpy(ref))


# ---- 2. match --------------------------------------------------------------------------------------------------------------------
def neg_form(box):
    """the same rectangle described with a negative width and height"""
    l, t, w, h = box
    return np.array([l + w, t + h, -w, -h], np.float32)


def undecidable(boxes_r, gt_r, nh, g, thresholds, eps=1e-9):
    for t in range(nh):
        v = [ref_box_iou(boxes_r[t], gt_r[j]) for j in range(g)]
        pos = [x for x in v if x > 0]
        if any(abs(x - float(np.float32(tau))) < eps for x in pos for tau in thresholds):
            return True
        if any(abs(a - b) < eps for i, a in enumerate(pos) for b in pos[i + 1:]):
            return True
    return False


def match_case(T, G, R, thresholds, seed):
    """Returns cont, owner, gt maps (16x16), boxes [T,R,4], num_objects, gt_boxes [R,G,4], gt_count, and the number of redraws."""
    rng = np.random.RandomState(seed)
    H = W = 16
    owner, gt = skewed_maps(rng, T, G, R, H, W)
    boxes, gt_boxes = np.zeros((T, R, 4), np.float32), np.zeros((R, G, 4), np.float32)
    num_objects, gt_count = np.zeros(R, np.int32), np.zeros(R, np.int32)
    redraws = 0
    for r in range(R):
        crafted = False
        while True:
            g = [0, G, G, 1, min(2, G), G][r] if r < 6 else int(rng.randint(0, G + 1))
            nh = [T, T, 0, T, T, T][r] if r < 6 else int(rng.randint(0, T + 1))
            gb = np.zeros((G, 4), np.float32)
            gb[:, :2] = rng.randint(0, 30, size=(G, 2))
            gb[:, 2:] = rng.randint(5, 21, size=(G, 2))
            pb = np.zeros((T, 4), np.float32)
            for t in range(T):
                base = gb[t % G] if t < 2 * G else np.array([rng.randint(0, 30), rng.randint(0, 30), rng.randint(5, 21), rng.randint(5, 21)])
                pb[t] = (base + rng.normal(0, 1.5, 4)).astype(np.float32)
                if rng.rand() < 0.3:
                    pb[t] = neg_form(pb[t])
            if r == 1:                                             # n^ and g at their maxima, asked for out of range: the clip
                nh, g = T + 3, G + 2
                pb[0] = gb[0]                                      # an exact duplicate of a ground-truth box: IoU == 1
                pb[1] = np.float32(np.nan)                         # one NaN row
            elif r == 2:
                nh, g = -2, G                                      # clipped to no prediction
            elif r == 3:
                pb[0] = gb[0] + np.array([0.5, 0.5, 0, 0], np.float32)   # IoU >= 0.68 for a box of 5 x 5 or more
                pb[1] = pb[0]                                      # two identical predictions for one ground truth
            elif r == 4 and G >= 2:
                gb[1] = gb[0]                                      # two identical ground-truth boxes: an exact tie, the smaller j wins
                crafted = True
            if r == 0:
                g = -1                                             # clipped to no ground truth
                gt[r] = -1
            if crafted or not undecidable(pb, gb, int(np.clip(nh, 0, T)), int(np.clip(g, 0, G)), thresholds):
                break
            redraws += 1
        boxes[:, r], gt_boxes[r], num_objects[r], gt_count[r] = pb, gb, nh, g
    # ARI edge cases in the maps
    if R > 3:
        gt[3] = -1; gt[3, 5, 5] = 0                                # a single foreground pixel
    if R > 4:
        gt[4] = -1; gt[4, 2:9, 3:8] = 0; owner[4, 2:9, 3:8] = 1 % T  # one object fully owned by one step
        owner[4, 12:, 12:] = 1 % T                                 # (which also owns pixels elsewhere)
    return ref_contingency(owner, gt, T, G), owner, gt, boxes, num_objects, gt_boxes, gt_count, redraws


@pytest.mark.parametrize("T,G,R", [(3, 2, 9), (5, 8, 6)])
@pytest.mark.parametrize("thresholds", [THRESHOLDS10, (0.5,)], ids=["K10", "K1"])
def test_match_against_f64_reference(gpu_device, T, G, R, thresholds):
    cases = 0
    redrawn = 0
    for seed in range(6):
        cont, owner, gt, boxes, n, gt_boxes, gc, redraws = match_case(T, G, R, thresholds, seed)
        cases += R
        redrawn += redraws
        ref = ref_match(cont, boxes, n, gt_boxes, gc, thresholds)
        d, out = run_match(cont, boxes, n, gt_boxes, gc, thresholds)
        check_match(out, ref)
        got_ari = out["ari"].cpu().numpy()
        # the crafted rows
        assert math.isnan(got_ari[0]) and got_ari[3] == 1.0 and got_ari[4] == 1.0
        assert out["box_iou"][1, 0, 0].item() == 1.0 and (out["box_iou"][1, 1] == 0).all()
        assert (out["match"][:, :, 2] == -1).all() and (out["best_overlap"][2] == 0).all() and out["count_err"][2].item() == -G
        assert (out["best_overlap"][0] == -1).all() and out["count_err"][0].item() == T
        m3 = out["match"][0, :2, 3].tolist()                       # identical predictions: the first takes the object, the second not
        assert m3[0] == 0 and m3[1] != 0
        if G >= 2:
            assert out["match"][0, 0, 4].item() in (0, -1) and ref["match"][0, 0, 4] != 1
        # ARI by pair counting over the pixels
        for r in range(R):
            pr = ref_ari_pairs(owner[r].reshape(-1), gt[r].reshape(-1))
            if math.isnan(pr):
                assert math.isnan(got_ari[r])
            else:
                assert abs(got_ari[r] - pr) <= TOL * (abs(pr) + 1), (r, got_ari[r], pr)
        # a second run gives the same bits
        _, again = run_match(cont, boxes, n, gt_boxes, gc, thresholds)
        for k in out:
            assert bits_equal(out[k], again[k]), k
    assert redrawn < 0.01 * cases, (redrawn, cases)


# ---- 3. reduce -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5, 1030])
def test_reduce_totals(gpu_device, R):
    T, G, K = 3, 2, 10
    rng = np.random.RandomState(R)
    nh, g = rng.randint(-1, T + 2, R).astype(np.int32), rng.randint(-1, G + 2, R).astype(np.int32)
    nhc, gc = np.clip(nh, 0, T), np.clip(g, 0, G)
    m = dict(count_err=(nhc - gc).astype(np.int32), ari=rng.uniform(-0.2, 1.0, R).astype(np.float32),
             best_overlap=rng.rand(R, G).astype(np.float32), box_iou=rng.rand(R, T, G).astype(np.float32),
             match=rng.randint(-1, G, (K, T, R)).astype(np.int8))
    m["ari"][rng.rand(R) < 0.2] = np.nan
    if R >= 5:
        m["ari"][3] = np.nan
    for r in range(R):
        m["match"][:, nhc[r]:, r] = -1
        m["best_overlap"][r, gc[r]:] = -1
    ti_ref, tf_ref = ref_totals(m, nh, g, T, G)
    d = dict(num_objects=torch.from_numpy(nh).cuda(), gt_count=torch.from_numpy(g).cuda())
    out = {k: torch.from_numpy(v).cuda() for k, v in m.items()}

    def run(acc, ti=None, tf=None):
        ti = torch.full((6 + K,), -99, dtype=torch.int64).cuda() if ti is None else ti
        tf = torch.full((3,), -99.0, dtype=torch.float64).cuda() if tf is None else tf
        run_reduce(d, out, T, G, K, ti, tf, acc)
        return ti, tf

    ti, tf = run(0)                                                # overwrites the sentinel
    assert ti.tolist() == ti_ref
    for got, ref in zip(tf.tolist(), tf_ref):
        assert abs(got - ref) <= 1e-12 * abs(ref), (got, ref)
    ti2, tf2 = run(0)
    assert torch.equal(ti, ti2) and bits_equal(tf, tf2)
    ti3, tf3 = run(1, ti2, tf2)                                    # accumulate: the integers double
    assert ti3.tolist() == [2 * v for v in ti_ref]
    assert torch.equal(tf3, tf + tf)                               # x + x is exact


# ---- 4. a perfect parse ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def glyphs():
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    return procedural_multi_mnist(32, seed=5, n_templates=200, return_annotations=True)


def test_ground_truth_as_its_own_prediction_scores_perfectly(gpu_device, glyphs):
    from attend_infer_repeat_amd.score import average_precision
    T, G, R = 3, 2, 32
    thresholds = THRESHOLDS10
    K = len(thresholds)
    counts = glyphs["nums"][:, :, 0].sum(0).astype(np.int32)
    inst = torch.from_numpy(glyphs["instances"]).cuda()
    boxes = np.zeros((T, R, 4), np.float32)
    boxes[:G] = glyphs["boxes"].transpose(1, 0, 2)
    cont = run_contingency(inst, inst, T, G)
    d, out = run_match(cont, boxes, counts, glyphs["boxes"], counts, thresholds)
    ti, tf = torch.zeros(6 + K, dtype=torch.int64).cuda(), torch.zeros(3, dtype=torch.float64).cuda()
    run_reduce(d, out, T, G, K, ti, tf, 0)
    ti, tf = ti.tolist(), tf.tolist()
    n_obj = int(counts.sum())
    assert 0 < n_obj and (counts == 0).any() and (counts == G).any()
    present = torch.arange(T)[:, None] < torch.from_numpy(counts)[None, :].long()
    assert ((out["match"].cpu() >= 0) == present[None]).all()
    ari = out["ari"].cpu()
    assert torch.equal(torch.isnan(ari), torch.from_numpy(counts == 0)) and (ari[~torch.isnan(ari)] == 1).all()
    assert ti[:6] == [R, R, 0, n_obj, n_obj, int((counts > 0).sum())] and ti[6:] == [n_obj] * K
    assert tf[1] == n_obj and tf[2] == n_obj and tf[0] == ti[5]
    score = (1.0 - 0.1 * torch.arange(T, dtype=torch.float32))[:, None].expand(T, R)      # decreasing in t
    keep = present.t().reshape(-1)
    for k in range(K):
        tp = (out["match"][k].cpu().t().reshape(-1) >= 0)[keep]
        assert float(average_precision(score.t().reshape(-1)[keep], tp, n_obj)) == 1.0


# ---- 5. end to end behind a SceneParser ------------------------------------------------------------------------------------------
def make_parser(name, R, seed=1):
    from oracle import air_oracle as O
    from test_engine import CONFIGS
    from test_parse import engine_config
    from attend_infer_repeat_amd.parse import SceneParser
    ocfg = CONFIGS[name][0]
    ps = SceneParser(engine_config(ocfg), R, seed=seed, mask_threshold=0.02)
    ps.load_parameters(O.init_params(ocfg, seed=1, bias_std=0.1))
    ps.set_global_step(20000)
    return ps, ocfg


def annotated_batches(name, R, n_batches, seed):
    """50x50: glyph canvases with the generator's annotations.  tiny (3x3 canvases, no room for a glyph): random maps and boxes."""
    if name == "mnist_b8":
        from attend_infer_repeat_amd.data import procedural_multi_mnist
        d = procedural_multi_mnist(R * n_batches, seed=seed, n_templates=200, return_annotations=True)
        imgs = d["imgs"].astype(np.float32) / 255.0
        return [dict(obs=imgs[i * R:(i + 1) * R], instances=d["instances"][i * R:(i + 1) * R], boxes=d["boxes"][i * R:(i + 1) * R])
                for i in range(n_batches)]
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n_batches):
        inst = (rng.randint(0, 3, (R, 3, 3)) - 1).astype(np.int8)
        boxes = np.zeros((R, 2, 4), np.float32)
        boxes[:, :, :2] = rng.randint(0, 2, (R, 2, 2))
        boxes[:, :, 2:] = rng.randint(1, 3, (R, 2, 2))
        boxes[rng.rand(R) < 0.4, 1] = 0                            # images with one object
        out.append(dict(obs=rng.rand(R, 3, 3).astype(np.float32), instances=inst, boxes=boxes))
    return out


def ref_batch(parsed, b, thresholds, T, G):
    """the numpy reference applied to the parser's RETURNED tensors"""
    owner = parsed["owner"].cpu().numpy()
    n = parsed["num_objects"].cpu().numpy()
    gc = (b["boxes"][:, :, 2] > 0).sum(1).astype(np.int32)
    cont = ref_contingency(owner, b["instances"], T, G)
    m = ref_match(cont, parsed["boxes"].cpu().numpy(), n, b["boxes"], gc, thresholds)
    stored = dict(m, **{k: m[k].astype(np.float32) for k in ("box_iou", "mask_iou", "ari", "best_overlap")})
    return cont, m, dict(m=stored, num_objects=n, gt_count=gc, score=parsed["score"].cpu().numpy())


@pytest.mark.parametrize("name,R,given", [("tiny", 10, None), ("mnist_b8", 8, None), ("mnist_b8", 8, "given")])
def test_scorer_matches_reference_over_two_batches(gpu_device, name, R, given):
    from attend_infer_repeat_amd.score import ParseScorer
    ps, ocfg = make_parser(name, R)
    T, G = ocfg.max_steps, 2
    thresholds = (0.3, 0.5, 0.75) if name == "tiny" else THRESHOLDS10
    sc = ParseScorer(ps, G, thresholds, max_batches=4)
    batches = annotated_batches(name, R, 2, seed=3)
    counts = None if given is None else torch.tensor([(i % 3) for i in range(R)], dtype=torch.int32).cuda()
    refs = []
    for i, b in enumerate(batches):
        parsed = ps.parse(torch.from_numpy(b["obs"]).cuda(), counts)
        got = sc.score(b["instances"], torch.from_numpy(b["boxes"]).cuda(), accumulate=i > 0)
        sc.synchronize()
        cont, m, rb = ref_batch(parsed, b, thresholds, T, G)
        refs.append(rb)
        assert torch.equal(got["cont"].cpu(), torch.from_numpy(cont))
        check_match(got, m)
        if given is not None:
            assert parsed["num_objects"].tolist() == counts.tolist()
        ti, tf = ref_totals(rb["m"], rb["num_objects"], rb["gt_count"], T, G) if i == 0 else (None, None)
        if i == 0:                                                 # accumulate=False: the totals are this batch's
            assert got["totals_i"].tolist() == ti
            close(got["totals_f"].cpu().numpy(), np.array(tf), 1e-12)
    same_summary(sc.summary(), ref_summary(refs, thresholds, T, G))
    # an explicit gt_count is used as given; reset() forgets everything
    sc.reset()
    gc = torch.zeros(R, dtype=torch.int32)
    got = sc.score(batches[0]["instances"], batches[0]["boxes"], gt_count=gc)
    sc.synchronize()
    assert (got["best_overlap"] == -1).all() and (got["match"] == -1).all()
    s = sc.summary()
    assert s["images"] == R and s["objects_gt"] == 0 and math.isnan(s["map"]) and math.isnan(s["mean_best_overlap"])
    with pytest.raises(ValueError, match="gt_boxes"):
        sc.score(batches[0]["instances"], batches[0]["boxes"][:, :1])
    for _ in range(3):
        sc.score(batches[0]["instances"], batches[0]["boxes"])
    with pytest.raises(ValueError, match="max_batches"):
        sc.score(batches[0]["instances"], batches[0]["boxes"])


def test_graph_replay_equals_eager_and_nothing_else_is_written(gpu_device):
    from attend_infer_repeat_amd.score import ParseScorer
    ps, ocfg = make_parser("mnist_b8", 8)
    eager, graph = ParseScorer(ps, 2), ParseScorer(ps, 2)
    graph.capture()
    batches = annotated_batches("mnist_b8", 8, 3, seed=9)
    eng = ps.engine
    state_keys = ("flat_params", "flat_ms", "flat_mg", "flat_mom", "step_dev", "rng_state")
    for i, b in enumerate(batches):
        live = ps.parse(torch.from_numpy(b["obs"]).cuda(), 2 if i == 1 else None)
        ps.synchronize()
        parsed = {k: v.clone() for k, v in live.items()}
        before = {k: getattr(eng, k).clone() for k in state_keys}
        acc = i != 1                                               # both accumulate values are replayed
        a = {k: v.clone() for k, v in eager.score(b["instances"], b["boxes"], accumulate=acc).items()}
        g = graph.score(b["instances"], b["boxes"], accumulate=acc)
        ps.synchronize()
        for k in a:
            assert bits_equal(a[k], g[k]), k
        for k in parsed:                                           # the parser's outputs and its engine are only read
            assert bits_equal(parsed[k], live[k]), k
        for k in state_keys:
            assert torch.equal(before[k], getattr(eng, k)), k
    sa, sg = eager.summary(), graph.summary()
    assert sa["images"] == 16 and set(sa) == set(sg)
    for k in sa:
        assert sa[k] == sg[k] or (math.isnan(sa[k]) and math.isnan(sg[k])), k
    graph.release_graphs()


# ---- 6. surface ------------------------------------------------------------------------------------------------------------------
EXPECTED_KEYS = ({"count_acc", "count_mae", "map", "fg_ari", "mean_best_overlap", "matched_box_iou", "images", "objects_pred",
                  "objects_gt"} | {"%s@%.2f" % (n, t) for n in ("precision", "recall", "f1", "ap") for t in THRESHOLDS10})


def test_score_parse_on_the_model_and_the_logger(gpu_device, tmp_path, capsys):
    from test_parse import _mnist_air, _train_state
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    from attend_infer_repeat_amd.evaluation import make_parse_score_logger
    B, T, G = 8, 3, 2
    air, ts, x, y = _mnist_air(B)
    ts()
    data = procedural_multi_mnist(2 * B, seed=7, n_templates=200, return_annotations=True)
    data = dict(data, imgs=data["imgs"].astype(np.float32) / 255.0)
    before = _train_state(air._engine)
    obs = torch.from_numpy(data["imgs"][:B]).cuda()
    got = air.score_parse(obs, data["instances"][:B], data["boxes"][:B])
    air._scene_parser.synchronize()
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert got is air.parse_scores and air.parse_scorer(G) is air._parse_scorer
    b = dict(obs=data["imgs"][:B], instances=data["instances"][:B], boxes=data["boxes"][:B])
    cont, m, rb = ref_batch(air.parsed, b, THRESHOLDS10, T, G)
    assert torch.equal(got["cont"].cpu(), torch.from_numpy(cont))
    check_match(got, m)
    # the logger: both batches in order, one line, one record
    path = os.path.join(tmp_path, "log.jsonl")
    with open(path, "w") as writer:
        acc = make_parse_score_logger(air, data, 2, "test", writer)(itr=4)
    refs = []
    for i in range(2):
        b = {k: data[kk][i * B:(i + 1) * B] for k, kk in (("obs", "imgs"), ("instances", "instances"), ("boxes", "boxes"))}
        refs.append(ref_batch(air.parse(torch.from_numpy(b["obs"]).cuda()), b, THRESHOLDS10, T, G)[2])
    same_summary(acc, ref_summary(refs, THRESHOLDS10, T, G))
    assert set(acc) == EXPECTED_KEYS
    printed = capsys.readouterr().out
    assert printed.count("Step 4, Data test parse score ") == 1 and "map = " in printed and "fg_ari = " in printed
    rec = [json.loads(l) for l in open(path)]
    assert len(rec) == 1 and rec[0]["data"] == "test_parse_score" and rec[0]["step"] == 4
    assert set(rec[0]) == EXPECTED_KEYS | {"step", "data"}


def test_training_script_parse_score_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    common = ["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "384", "--eval-batches", "1",
              "--summary-every", "0", "--parse-score"]
    # refused before any training step when the data has no annotations
    with pytest.raises(SystemExit):
        multi_mnist.main(common + ["--results-dir", os.path.join(tmp_path, "refused")])
    assert "annotat" in capsys.readouterr().err
    assert not os.path.exists(os.path.join(tmp_path, "refused", "multi_mnist", "log.jsonl"))
    air = multi_mnist.main(common + ["--glyphs", "--results-dir", str(tmp_path)])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_parse_score"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count(" parse score ") == 2
    for l in rec:
        assert l["images"] == 64 and 0.0 <= l["count_acc"] <= 1.0 and set(l) == EXPECTED_KEYS | {"step", "data"}
