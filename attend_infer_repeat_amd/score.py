"""Scoring scene parses against ground truth on the device: detection (precision, recall, F1 and AP over box-IoU thresholds) and
segmentation (foreground ARI, mean best overlap) figures over a validation set, next to the count accuracy.

`ParseScorer` binds to a `SceneParser`'s output tensors (their addresses never change) and appends three launches of libair_hip.so
(include/air_hip.h describes them) behind a parse, on the parser's engine stream:

  air_score_contingency  cont[r, a, b] = #pixels with owner + 1 == a and gt + 1 == b: the one pass over the R * H * W maps;
  air_score_match        per image from cont and the boxes: box IoU and mask IoU of every (step, object) pair, the greedy PASCAL / COCO
                         assignment per threshold in step order (= score order: score[t] = q(n > t) is non-increasing in t), foreground
                         ARI, the best overlap of every ground-truth object, the count error;
  air_score_reduce       the sums over the batch, added to device-resident totals: a validation loop reads back once, in `summary()`.

AP needs every prediction of the set, so score, presence and match of each call are kept in preallocated device buffers of
`max_batches` rows (a device-to-device copy per call, no host synchronisation); `average_precision` sorts them once in `summary()`.
The parser and its engine are read, never written.
"""
from typing import Dict, Sequence

from .launch import destroy_graphs

DEFAULT_THRESHOLDS = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))
MAX_GT_OBJECTS, MAX_THRESHOLDS = 8, 16


def check_arguments(max_gt_objects, thresholds) -> None:
    """Refuse what the kernels have no room for (pure host code: importable and callable without a GPU)."""
    g = int(max_gt_objects)
    if g != max_gt_objects or not 1 <= g <= MAX_GT_OBJECTS:
        raise ValueError("max_gt_objects must be in 1..%d, got %r" % (MAX_GT_OBJECTS, max_gt_objects))
    th = [float(t) for t in thresholds]
    if not 1 <= len(th) <= MAX_THRESHOLDS:
        raise ValueError("thresholds: between 1 and %d values, got %d" % (MAX_THRESHOLDS, len(th)))
    if any(not (0.0 < t <= 1.0) for t in th):
        raise ValueError("thresholds must lie in (0, 1], got %r" % (th,))
    if any(b <= a for a, b in zip(th, th[1:])):
        raise ValueError("thresholds must be strictly increasing, got %r" % (th,))


def average_precision(scores, tp, n_gt):
    """All-point interpolated AP of a set of predictions (runs on whatever device holds them, CPU included).
    scores [N], tp [N] (true-positive flags), n_gt: the number of ground-truth objects.  Predictions with a NaN score are not
    valid and drop out; the rest are sorted by descending score with a STABLE sort, so arrival order breaks ties; precision and
    recall are cumulative in float64; AP = sum_i (r_i - r_{i-1}) * max_{j >= i} p_j.  NaN when n_gt == 0.  Returns a 0-dim float64
    tensor."""
    import torch
    scores = torch.as_tensor(scores).reshape(-1)
    tp = torch.as_tensor(tp, device=scores.device).reshape(-1)
    if int(n_gt) == 0:
        return torch.full((), float("nan"), dtype=torch.float64, device=scores.device)
    valid = ~torch.isnan(scores.double())
    scores, tp = scores[valid], tp[valid]
    if scores.numel() == 0:
        return torch.zeros((), dtype=torch.float64, device=scores.device)
    order = torch.argsort(scores, descending=True, stable=True)
    hits = torch.cumsum(tp[order].to(torch.float64), 0)
    precision = hits / torch.arange(1, hits.numel() + 1, dtype=torch.float64, device=scores.device)
    recall = hits / float(n_gt)
    envelope = torch.flip(torch.cummax(torch.flip(precision, (0,)), 0).values, (0,))
    steps = recall - torch.cat([torch.zeros(1, dtype=torch.float64, device=scores.device), recall[:-1]])
    return (steps * envelope).sum()


def threshold_key(name: str, tau: float) -> str:
    return "%s@%.2f" % (name, tau)


class ParseScorer:
    def __init__(self, parser, max_gt_objects: int, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, max_batches: int = 256):
        check_arguments(max_gt_objects, thresholds)
        if int(max_batches) < 1:
            raise ValueError("max_batches must be >= 1, got %r" % (max_batches,))
        import torch
        from . import hip as H
        self.parser = parser
        self.G, self.thresholds_host = int(max_gt_objects), tuple(float(t) for t in thresholds)
        self.K, self.max_batches = len(self.thresholds_host), int(max_batches)
        eng = parser.engine
        self.T, self.R = parser.T, parser.R
        T, R, G, K = self.T, self.R, self.G, self.K
        Hi, Wi = parser.owner.shape[1:]
        dev = eng.device
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.gt_instances, self.gt_boxes, self.gt_count = z((R, Hi, Wi), torch.int8), z((R, G, 4)), z((R,), torch.int32)
            self.thresholds = torch.tensor(self.thresholds_host, dtype=torch.float32, device=dev)
            self.cont = z((R, T + 1, G + 1), torch.int32)
            self.box_iou, self.mask_iou = z((R, T, G)), z((R, T, G))
            self.match = z((K, T, R), torch.int8)
            self.ari, self.best_overlap, self.count_err = z((R,)), z((R, G)), z((R,), torch.int32)
            self.totals_i, self.totals_f = z((6 + K,), torch.int64), z((3,), torch.float64)
            self.ap_score, self.ap_presence = z((self.max_batches, T, R)), z((self.max_batches, T, R))
            self.ap_match = z((self.max_batches, K, T, R), torch.int8)
        self.calls = 0
        self._graphs = {}
        L, p = H.lib(), H._p
        head = [(L.air_score_contingency, (p(parser.owner), p(self.gt_instances), T, G, R, int(Hi), int(Wi), p(self.cont)),
                 "air_score_contingency"),
                (L.air_score_match, (p(self.cont), p(parser.boxes), p(parser.num_objects), p(self.gt_boxes), p(self.gt_count),
                                     p(self.thresholds), T, G, K, R, p(self.box_iou), p(self.mask_iou), p(self.match), p(self.ari),
                                     p(self.best_overlap), p(self.count_err)), "air_score_match")]
        reduce = lambda acc: (L.air_score_reduce, (p(parser.num_objects), p(self.gt_count), p(self.count_err), p(self.ari),
                                                   p(self.best_overlap), p(self.match), p(self.box_iou), T, G, K, R, p(self.totals_i),
                                                   p(self.totals_f), acc), "air_score_reduce")
        self._plans = {acc: head + [reduce(int(acc))] for acc in (False, True)}
        eng.synchronize()

    # ---- graphs -------------------------------------------------------------------------------------------------------------
    def capture(self):
        """the three launches as ONE hipGraph per `accumulate` value"""
        self.release_graphs()
        eng = self.parser.engine
        eng.synchronize()
        for key, plan in self._plans.items():
            self._graphs[key] = eng._capture_plans([plan])

    def release_graphs(self):
        destroy_graphs(self._graphs.values())
        self._graphs = {}

    def reset(self):
        """zero the totals and forget the predictions kept for AP"""
        import torch
        eng = self.parser.engine
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            for t in (self.totals_i, self.totals_f, self.ap_score, self.ap_presence, self.ap_match):
                t.zero_()
        self.calls = 0

    # ---- one batch ----------------------------------------------------------------------------------------------------------
    def score(self, gt_instances, gt_boxes, gt_count=None, accumulate: bool = True) -> Dict[str, object]:
        """Score the parser's LATEST parse against gt_instances [R, H, W] (int8, -1 = background), gt_boxes [R, G, 4] (left, top,
        width, height) and gt_count [R] (None: the number of rows of gt_boxes with width > 0).  accumulate=False restarts the
        totals (and the predictions kept for AP) with this batch.  Returns device tensors that the NEXT call overwrites: cont
        [R, T+1, G+1] int32, box_iou, mask_iou [R, T, G], match [K, T, R] int8, ari [R], best_overlap [R, G], count_err [R] int32,
        totals_i [6+K] int64, totals_f [3] float64.  The launches go through launch.run_plan (or the captured graph) on the parser's engine stream; on return the caller's current
        stream is ordered after it, and the next call waits for the caller's reads before it overwrites them."""
        import torch
        eng, R, G = self.parser.engine, self.R, self.G
        gi, gb = torch.as_tensor(gt_instances), torch.as_tensor(gt_boxes)
        if tuple(gi.shape) != tuple(self.gt_instances.shape):
            raise ValueError("gt_instances: expected %s, got %s" % (tuple(self.gt_instances.shape), tuple(gi.shape)))
        if tuple(gb.shape) != (R, G, 4):
            raise ValueError("gt_boxes: expected %s, got %s" % ((R, G, 4), tuple(gb.shape)))
        gc = None if gt_count is None else torch.as_tensor(gt_count).reshape(-1)
        if gc is not None and gc.numel() != R:
            raise ValueError("gt_count: one count per image (%d), got %d" % (R, gc.numel()))
        if not accumulate:
            self.calls = 0
        if self.calls >= self.max_batches:
            raise ValueError("ParseScorer keeps the predictions of at most max_batches = %d calls for AP; reset() or build it "
                             "with more" % self.max_batches)
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            self.gt_instances.copy_(gi, non_blocking=True)
            self.gt_boxes.copy_(gb, non_blocking=True)
            if gc is not None:
                self.gt_count.copy_(gc, non_blocking=True)
            else:
                self.gt_count.copy_((self.gt_boxes[..., 2] > 0).sum(-1))
        for t in (gi, gb, gc):
            if t is not None and t.is_cuda:
                t.record_stream(eng.stream)
        key = bool(accumulate)
        eng._replay_or_run(self._graphs.get(key), self._plans[key])
        with torch.cuda.stream(eng.stream):
            i = self.calls
            self.ap_score[i].copy_(self.parser.score, non_blocking=True)
            self.ap_presence[i].copy_(self.parser.presence, non_blocking=True)
            self.ap_match[i].copy_(self.match, non_blocking=True)
        self.calls += 1
        eng.wait_for_engine()
        return {"cont": self.cont, "box_iou": self.box_iou, "mask_iou": self.mask_iou, "match": self.match, "ari": self.ari,
                "best_overlap": self.best_overlap, "count_err": self.count_err, "totals_i": self.totals_i,
                "totals_f": self.totals_f}

    # ---- the set ------------------------------------------------------------------------------------------------------------
    def summary(self) -> Dict[str, float]:
        """The figures of everything scored since the last reset (ONE readback): count_acc, count_mae, precision@t / recall@t / f1@t /
        ap@t per threshold and map (their mean), fg_ari (mean over the images with foreground), mean_best_overlap (over the
        ground-truth objects), matched_box_iou (mean box IoU of the pairs matched at the first threshold), images, objects_pred,
        objects_gt.  A figure without a denominator is NaN."""
        import torch
        eng, K, n = self.parser.engine, self.K, self.calls
        eng.wait_for_engine()
        # predictions in arrival order: (batch, image, step)
        keep = self.ap_presence[:n].permute(0, 2, 1).reshape(-1) > 0.5
        scores = self.ap_score[:n].permute(0, 2, 1).reshape(-1)[keep]
        tp = (self.ap_match[:n].permute(1, 0, 3, 2).reshape(K, -1) >= 0)[:, keep]
        n_gt_dev = self.totals_i[4]
        aps = []
        order = torch.argsort(scores, descending=True, stable=True) if scores.numel() else None
        for k in range(K):                                         # (average_precision's arithmetic with the sort shared and n_gt on the device)
            if order is None:
                aps.append(torch.where(n_gt_dev > 0, torch.zeros_like(self.totals_f[0]), float("nan")))
                continue
            hits = torch.cumsum(tp[k][order].to(torch.float64), 0)
            precision = hits / torch.arange(1, hits.numel() + 1, dtype=torch.float64, device=hits.device)
            recall = hits / n_gt_dev.double()
            envelope = torch.flip(torch.cummax(torch.flip(precision, (0,)), 0).values, (0,))
            steps = recall - torch.cat([torch.zeros(1, dtype=torch.float64, device=hits.device), recall[:-1]])
            aps.append(torch.where(n_gt_dev > 0, (steps * envelope).sum(), float("nan")))
        flat = torch.cat([self.totals_i.double(), self.totals_f, torch.stack(aps).reshape(-1)]).tolist()      # the readback
        ti, tf, ap = [int(v) for v in flat[:6 + K]], flat[6 + K:9 + K], flat[9 + K:]
        div = lambda a, b: a / b if b else float("nan")
        images, correct, abs_err, n_pred, n_gt, n_ari = ti[:6]
        out = {"count_acc": div(correct, images), "count_mae": div(abs_err, images)}
        for k, tau in enumerate(self.thresholds_host):
            pr, rc = div(ti[6 + k], n_pred), div(ti[6 + k], n_gt)
            out[threshold_key("precision", tau)], out[threshold_key("recall", tau)] = pr, rc
            out[threshold_key("f1", tau)] = div(2 * ti[6 + k], n_pred + n_gt)
            out[threshold_key("ap", tau)] = ap[k]
        out["map"] = sum(ap) / K
        out.update(fg_ari=div(tf[0], n_ari), mean_best_overlap=div(tf[1], n_gt), matched_box_iou=div(tf[2], ti[6]),
                   images=images, objects_pred=n_pred, objects_gt=n_gt)
        return out

    def synchronize(self):
        self.parser.engine.synchronize()
