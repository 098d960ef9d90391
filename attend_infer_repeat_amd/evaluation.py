"""Logging / evaluation helpers with the interface of the reference's evaluation.py (make_logger, make_expr_logger,
rect_stn, make_fig; attend_infer_repeat/evaluation.py:14-166).  Pure consumers of the model's attributes: no kernels
here.  TensorBoard summaries are replaced by returned dicts (and an optional JSON-lines file); figures need matplotlib.
"""
import json
import time


def attention_box(stn_params, width, height):
    """Pixel rectangle (left, top, box_width, box_height) that the glimpse of [sx, tx, sy, ty] covers on a width x height
    canvas.  This is the only in-tree statement of the reference's spatial-transformer convention (evaluation.py:23-28): the
    glimpse spans sx (sy) of the canvas extent and its centre sits tx (ty) half-extents away from the canvas centre."""
    sx, tx, sy, ty = (float(v) for v in stn_params)
    return width * (1. - sx + tx) / 2, height * (1. - sy + ty) / 2, width * sx, height * sy


def rect_stn(ax, width, height, stn_params, c=None, line_width=3):
    """Draw the attention box of one glimpse on `ax` (pixel centres at integer coordinates, hence the half-pixel shift)."""
    from matplotlib.patches import Rectangle
    left, top, bw, bh = attention_box(stn_params, width, height)
    patch = Rectangle((left - .5, top - .5), bw, bh, linewidth=line_width, edgecolor=c, facecolor='none')
    ax.add_patch(patch)
    return patch


def _figure_tensors(air):
    """what the progress figure shows, as host arrays"""
    host = lambda t: t.detach().cpu().numpy()
    step_probs = None
    if hasattr(air, "num_steps_distrib"):
        step_probs = host(air.num_steps_distrib.prob()[..., 1:])          # [B, T]: p(n = t + 1)
    return dict(obs=host(air.obs), canvas=host(air.canvas), glimpse=host(air.glimpse), presence=host(air.presence)[..., 0],
                where=host(air.where), step_probs=step_probs)


def make_fig(air, checkpoint_dir=None, global_step=None, n_samples=10):
    """Progress figure with the content of the reference's (evaluation.py:31-65): one column per sample; the first row shows the
    input, the next max_steps rows the canvas after each step with the attention box of every step that is present, the last
    max_steps rows the glimpse each step reconstructed, titled with the sampled presence and the posterior probability of that
    step count.  Saved as progress_fig_<global_step>.png when a directory is given."""
    import os.path as osp
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    d = _figure_tensors(air)
    T = air.max_steps
    cols = min(n_samples, air.batch_size)
    img_h, img_w = d["obs"].shape[1:]
    inch = 1.5
    fig, axes = plt.subplots(2 * T + 1, cols, figsize=(inch * cols, inch * (2 * T + 1)), squeeze=False)
    for col in range(cols):
        axes[0][col].imshow(d["obs"][col], cmap='gray', vmin=0, vmax=1)
        for t in range(T):
            canvas_ax, glimpse_ax = axes[1 + t][col], axes[1 + T + t][col]
            canvas_ax.imshow(d["canvas"][t, col], cmap='gray', vmin=0, vmax=1)
            if d["presence"][t, col] > .5:
                rect_stn(canvas_ax, img_w, img_h, d["where"][t, col], 'r')
            glimpse_ax.imshow(d["glimpse"][t, col], cmap='gray')
            if d["step_probs"] is not None:
                glimpse_ax.set_title('{:d} with p({:d}) = {:.02f}'.format(int(d["presence"][t, col]), t + 1,
                                                                         float(d["step_probs"][col, t])), fontsize=4 * inch)
    for ax in axes.ravel():
        ax.set_axis_off()
    if checkpoint_dir is not None:
        fig.savefig(osp.join(checkpoint_dir, 'progress_fig_{}.png'.format(global_step)), dpi=300)
        plt.close(fig)
    return fig


def make_prior_fig(air, checkpoint_dir=None, global_step=None, n_samples=10, count_probs="uniform"):
    """Scenes drawn from the generative model (air.sample_scenes with `count_probs`; the sampler keeps the size it has): one column
    per scene; the first row shows the mean canvas with the attention box of every step that is present, the next max_steps rows
    the glimpse each step decoded, titled with its presence.  The caption names the count distribution.  Saved as
    prior_fig_<global_step>.png when a directory is given."""
    import os.path as osp
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    air.sample_scenes(count_probs=count_probs)
    host = lambda t: t.detach().cpu().numpy()
    mean, glimpse = host(air.generated_mean), host(air.generated_glimpse)
    presence, where = host(air.generated_presence), host(air.generated_where)
    T = air.max_steps
    cols = min(n_samples, mean.shape[0])
    img_h, img_w = mean.shape[1:]
    inch = 1.5
    fig, axes = plt.subplots(T + 1, cols, figsize=(inch * cols, inch * (T + 1)), squeeze=False)
    for col in range(cols):
        axes[0][col].imshow(mean[col], cmap='gray', vmin=0, vmax=1)
        for t in range(T):
            if presence[t, col] > .5:
                rect_stn(axes[0][col], img_w, img_h, where[t, col], 'r')
            axes[1 + t][col].imshow(glimpse[t, col], cmap='gray')
            axes[1 + t][col].set_title('{:d}'.format(int(presence[t, col])), fontsize=4 * inch)
    for ax in axes.ravel():
        ax.set_axis_off()
    fig.suptitle('prior samples, count distribution: {}'.format(air.scene_sampler().count_label), fontsize=5 * inch)
    if checkpoint_dir is not None:
        fig.savefig(osp.join(checkpoint_dir, 'prior_fig_{}.png'.format(global_step)), dpi=300)
        plt.close(fig)
    return fig


def make_parse_fig(air, checkpoint_dir=None, global_step=None, n_samples=10, obs=None, particles=None, select="joint"):
    """The parse of a batch (air.parse; particles=None: the deterministic parse at the mode, particles=K: the best of K posterior
    particles under `select`): one column per image; the input, the reconstruction with the attention box of every object the parse
    found (rect_stn), and the owner map (which object a pixel belongs to; background = -1).  Saved as parse_fig_<global_step>.png
    when a directory is given."""
    import os.path as osp
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    out = air.parse(obs) if particles is None else air.parse(obs, particles=particles, select=select)
    host = lambda t: t.detach().cpu().numpy()
    x, rec, owner = host(air.obs), host(out["reconstruction"]), host(out["owner"])
    presence, where, count_prob = host(out["presence"]), host(out["where"]), host(out["count_prob"])
    T = presence.shape[0]
    cols = min(n_samples, x.shape[0])
    img_h, img_w = x.shape[1:]
    inch = 1.5
    fig, axes = plt.subplots(3, cols, figsize=(inch * cols, inch * 3), squeeze=False)
    colours = plt.get_cmap('tab10')
    for col in range(cols):
        axes[0][col].imshow(x[col], cmap='gray', vmin=0, vmax=1)
        axes[1][col].imshow(rec[col], cmap='gray', vmin=0, vmax=1)
        for t in range(T):
            if presence[t, col] > .5:
                rect_stn(axes[1][col], img_w, img_h, where[t, col], colours(t % 10), line_width=1)
        axes[1][col].set_title('n = {:d}, q = {:.02f}'.format(int(presence[:, col].sum()), float(count_prob[col])), fontsize=4 * inch)
        axes[2][col].imshow(owner[col], cmap='tab10', vmin=-1, vmax=max(T - 1, 8), interpolation='nearest')
    for ax in axes.ravel():
        ax.set_axis_off()
    if checkpoint_dir is not None:
        fig.savefig(osp.join(checkpoint_dir, 'parse_fig_{}.png'.format(global_step)), dpi=300)
        plt.close(fig)
    return fig


def _particle_sums(out):
    """[number of images whose kept particle is not particle 0, sum of the effective sample size]"""
    return [(out["best_particle"] != 0).double().sum(), out["ess"].double().sum()]


def _refine_sums(out):
    """[sum of the objective gain, number of images whose best iterate is not the start parse] (an image whose gain is NaN or
    infinite adds 0; the callers divide by the number of all images)"""
    import torch
    obj, obj0 = out.get("refine_objective", out["objective"]), out.get("refine_objective_start", out["objective_start"])      # (behind a pruner)
    gain = torch.nan_to_num(obj - obj0.double(), nan=0.0, posinf=0.0, neginf=0.0)
    return [gain.sum(), (out["best_iter"] > 0).double().sum()]


def _prune_sums(out):
    """[number of images whose count changed, objects dropped, objects added, sum of the objective gain] of a pruned parse (an image
    whose gain is NaN or infinite adds 0; the callers divide by the number of all images)"""
    import torch
    best, m0 = out["best_mask"].to(torch.int64), (1 << out["num_objects_start"].to(torch.int64)) - 1
    bits = lambda m: sum((m >> t) & 1 for t in range(out["kept_step"].shape[0]))
    gain = torch.nan_to_num(out["objective"] - out["objective_start"].double(), nan=0.0, posinf=0.0, neginf=0.0)
    return [(out["num_objects"] != out["num_objects_start"]).double().sum(), bits(m0 & ~best).double().sum(),
            bits(best & ~m0).double().sum(), gain.sum()]


def _propose_sums(out):
    """[objects of the result that came from a proposal, number of images whose count changed, sum of the objective gain] of a parse
    behind residual proposals (an image whose gain is NaN or infinite adds 0; the callers divide by the number of all images)"""
    import torch
    gain = torch.nan_to_num(out["objective"] - out["objective_start"].double(), nan=0.0, posinf=0.0, neginf=0.0)
    return [out["objects_proposed_kept"].double().sum(), (out["num_objects"] != out["num_objects_start"]).double().sum(), gain.sum()]


class _ParseExtras:
    """What a parse carries on top of the plain one -- particles, refine, prune, propose -- as the parse loggers need it: `kw`, the
    keyword arguments of air.parse / parse_scorer / score_parse (plain ints, lists and tuples, so that the record can be written);
    `suffix`, what the label of the line says about them; start(device) / add(out) / figures(n_images), the sums of their figures
    over the parses `out` in float64 on the device and the means per image by name.  The gain of the subset search is objective_gain,
    prune_objective_gain / propose_objective_gain next to refine=N, whose own gain keeps the name."""

    def __init__(self, particles, select, refine, refine_lr, prune, propose):
        self.kw, self.suffix, self.sums, self.names = {}, '', [], []
        gain = "objective_gain"
        if particles is not None:
            self.kw.update(particles=int(particles), select=select)
            self.suffix += '({}, {})'.format(int(particles), select)
            self._figures(_particle_sums, "best_particle_moved", "ess")
        if refine is not None:
            self.kw["refine"] = int(refine)
            if refine_lr is not None:
                self.kw["refine_lr"] = tuple(float(v) for v in refine_lr)
            self.suffix += '+refine({})'.format(int(refine))
            self._figures(_refine_sums, gain, "refine_moved")
        if prune is not None:
            self.kw["prune"] = prune
            self.suffix += '+prune({})'.format(prune)
            self._figures(_prune_sums, "count_changed", "objects_dropped", "objects_added", gain if refine is None else "prune_" + gain)
        if propose is not None:
            self.kw["propose"] = [int(v) for v in propose] if isinstance(propose, (tuple, list)) else int(propose)
            self.suffix += '+propose({})'.format(self.kw["propose"])
            self._figures(_propose_sums, "objects_added_from_residual", "count_changed", gain if refine is None else "propose_" + gain)

    def _figures(self, sums, *names):
        self.sums.append(sums)
        self.names += names

    def start(self, device):
        import torch
        self.total = torch.zeros(len(self.names), dtype=torch.float64, device=device)

    def add(self, out):
        import torch
        if self.sums:
            self.total += torch.stack([v for sums in self.sums for v in sums(out)])

    def figures(self, n_images):
        return dict(zip(self.names, (self.total / n_images).tolist()))


def make_parse_logger(air, data_fn, num_batches, name, writer=None, measure_time=True, particles=None, select="joint", refine=None,
                      refine_lr=None, prune=None, propose=None):
    """The deterministic parse (air.parse: the mode of q(n | x), latents at their posterior means) over `num_batches` batches from
    `data_fn`: map_num_step_acc (the count against the true one), the mean count_prob (q at the mode) and the mean number of
    objects per image.  particles=K: the best of K posterior particles under `select` instead (the count and count_prob are then
    the kept particle's), and two more figures: best_particle_moved (the share of images whose kept particle is not particle 0)
    and ess (the mean effective sample size); the record names K and the criterion.  refine=N: that parse refined by N gradient
    iterations (air.parse(refine=N, refine_lr=...)), and two more figures: objective_gain (the mean of objective - objective_start
    over ALL images, an image whose gain is not finite counting as 0) and refine_moved (the share of images whose best iterate is not the start parse); the
    record names N.  prune="present" | "all": that parse behind the subset search (air.parse(prune=...)), and count_changed (the share
    of images with num_objects != num_objects_start), objects_dropped and objects_added (means per image) and objective_gain (as
    above, of the subset search: objective - objective_start of the pruner; together with refine=N it is reported as
    prune_objective_gain, objective_gain stays the refiner's); the record names the mode.  propose=P | (P, rounds): that parse behind
    residual proposals (air.parse(propose=...); not together with prune), and objects_added_from_residual (objects of the result that
    came from a proposal, mean per image), count_changed and objective_gain (of the proposer; propose_objective_gain next to
    refine=N); the record names the spec.  Prints / writes one line like make_expr_logger."""
    import torch
    extras = _ParseExtras(particles, select, refine, refine_lr, prune, propose)

    def logger(itr=0, num_batches_to_eval=None, write=True):
        n = num_batches if num_batches_to_eval is None else num_batches_to_eval
        n = max(int(n), 1)
        start = time.time()
        tot = torch.zeros(3, dtype=torch.float64, device=air.obs.device)
        extras.start(air.obs.device)
        images = 0
        for _ in range(n):
            obs, nums = data_fn()
            out = air.parse(obs, **extras.kw)
            gt = nums.sum(0).reshape(-1).to(torch.int64)
            cnt = out["num_objects"].to(torch.int64)
            tot += torch.stack([(cnt == gt).double().sum(), out["count_prob"].double().sum(), cnt.double().sum()])
            extras.add(out)
            images += int(cnt.numel())
        acc = dict(zip(("map_num_step_acc", "count_prob", "num_objects"), (tot / images).tolist()), **extras.figures(images))
        t = time.time() - start
        msg = 'Step {}, Data {} parse{} '.format(itr, name, extras.suffix) + ', '.join('{} = {:.4f}'.format(k, v) for k, v in acc.items())
        if measure_time:
            msg += ', eval time = {:.4}s'.format(t)
        print(msg)
        if write and writer is not None:
            writer.write(json.dumps(dict(step=int(itr), data=name + "_parse", **extras.kw, **acc)) + "\n"); writer.flush()
        return acc
    return logger


def make_parse_score_logger(air, data, num_batches, name, writer=None, thresholds=None, measure_time=True, particles=None,
                            select="joint", refine=None, refine_lr=None, prune=None, propose=None):
    """The deterministic parse scored against the generator's annotations on the device (air.score_parse, score.ParseScorer):
    `data` is an annotated dataset dict (imgs [N, H, W], boxes [N, G, 4], instances [N, H, W] int8 -- data.create_multi_mnist with
    return_annotations=True), walked in order from its start in `num_batches` batches of the model's size (fewer when the data
    runs out).  The sums and the predictions AP needs stay on the device; ParseScorer.summary() is the one readback.  Prints /
    writes one line like make_parse_logger: count accuracy, precision / recall / F1 / AP per box-IoU threshold and their mean AP,
    foreground ARI, mean best overlap.  particles=K: the best of K posterior particles under `select` is scored instead; the line
    also reports best_particle_moved and ess as make_parse_logger does, and the record names K and the criterion.  refine=N: the
    refined parse is scored; the line also reports objective_gain and refine_moved as make_parse_logger does.  prune=...: the pruned
    parse is scored; the line also reports count_changed, objects_dropped, objects_added and objective_gain (prune_objective_gain
    next to refine=N) as make_parse_logger does.  propose=...: the parse behind residual proposals is scored; the line also reports
    objects_added_from_residual, count_changed and objective_gain (propose_objective_gain next to refine=N) as make_parse_logger does."""
    import torch
    G = int(data["boxes"].shape[1])
    kw = {} if thresholds is None else dict(thresholds=tuple(thresholds))
    extras = _ParseExtras(particles, select, refine, refine_lr, prune, propose)

    def logger(itr=0, num_batches_to_eval=None, write=True):
        n = num_batches if num_batches_to_eval is None else num_batches_to_eval
        B = int(air.obs.shape[0])
        n = min(max(int(n), 1), int(data["imgs"].shape[0]) // B)
        if n < 1:
            raise ValueError("the annotated dataset holds fewer images than one batch of %d" % B)
        start = time.time()
        dev = air.obs.device
        scorer = air.parse_scorer(G, **kw, **extras.kw)
        scorer.reset()
        extras.start(dev)
        for i in range(n):
            sl = slice(i * B, (i + 1) * B)
            air.score_parse(torch.as_tensor(data["imgs"][sl], dtype=torch.float32).to(dev), torch.as_tensor(data["instances"][sl]),
                            torch.as_tensor(data["boxes"][sl]), **kw, **extras.kw)
            extras.add(air.parsed)
        acc = scorer.summary()
        acc.update(extras.figures(n * B))
        shown = ["count_acc", "map", "ap@%.2f" % scorer.thresholds_host[0], "fg_ari", "mean_best_overlap", "matched_box_iou"] + extras.names
        t = time.time() - start
        msg = 'Step {}, Data {} parse score{} '.format(itr, name, extras.suffix) + ', '.join('{} = {:.4f}'.format(k, acc[k]) for k in shown)
        if measure_time:
            msg += ', eval time = {:.4}s'.format(t)
        print(msg)
        if write and writer is not None:
            writer.write(json.dumps(dict(step=int(itr), data=name + "_parse_score", **extras.kw, **acc)) + "\n"); writer.flush()
        return acc
    return logger


def make_tiled_parse_fig(air, scenes, checkpoint_dir=None, global_step=None, n_samples=4, stride=None, iou_merge=0.5, **parse_kw):
    """The tiled parse of scenes larger than the canvas (air.parse_tiled): one column per scene; the scene, the reconstruction with
    the window grid (thin lines) and the attention box of every kept object coloured by the WINDOW it came from (rect_stn on the
    scene-frame `where`), and the owner map (which object a pixel belongs to; background = -1).  Saved as
    tiled_parse_fig_<global_step>.png when a directory is given."""
    import os.path as osp
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    import torch
    from .tile import window_origins
    out = air.parse_tiled(scenes, stride=stride, iou_merge=iou_merge, **parse_kw)
    host = lambda t: t.detach().cpu().numpy()
    x, rec, owner = host(torch.as_tensor(scenes)), host(out["reconstruction"]), host(out["owner"])
    presence, where, kept, counts = host(out["presence"]), host(out["where"]), host(out["kept_cand"]), host(out["merge_counts"])
    C = presence.shape[0]
    cols = min(n_samples, x.shape[0])
    Hs, Ws = x.shape[1:]
    H, W = out["windows"].shape[1:]
    T = out["cand_state"].shape[1] // out["window_num_objects"].shape[1]
    oy, ox = window_origins((Hs, Ws), (H, W), stride)
    inch = 2.5
    fig, axes = plt.subplots(3, cols, figsize=(inch * cols * Ws / max(Hs, Ws), inch * 3 * Hs / max(Hs, Ws)), squeeze=False)
    colours = plt.get_cmap('tab20')
    for col in range(cols):
        axes[0][col].imshow(x[col], cmap='gray', vmin=0, vmax=1)
        axes[1][col].imshow(rec[col], cmap='gray', vmin=0, vmax=1)
        for y in oy:
            for xo in ox:
                axes[1][col].add_patch(plt.Rectangle((xo - .5, y - .5), W, H, fill=False, lw=.3, ec='white', alpha=.4))
        for j in range(C):
            if presence[j, col] > .5:
                rect_stn(axes[1][col], Ws, Hs, where[j, col], colours((int(kept[j, col]) // T) % 20), line_width=1)
        axes[1][col].set_title('n = {:d}, dup = {:d}, not owned = {:d}'.format(int(presence[:, col].sum()), int(counts[col, 3]),
                                                                               int(counts[col, 2])), fontsize=3 * inch)
        axes[2][col].imshow(owner[col], cmap='tab20', vmin=-1, vmax=max(C - 1, 18), interpolation='nearest')
    for ax in axes.ravel():
        ax.set_axis_off()
    if checkpoint_dir is not None:
        fig.savefig(osp.join(checkpoint_dir, 'tiled_parse_fig_{}.png'.format(global_step)), dpi=300)
        plt.close(fig)
    return fig


def make_tiled_parse_score_logger(air, data, num_batches, name, batch_size=None, writer=None, thresholds=None, measure_time=True,
                                  stride=None, iou_merge=0.5, refine=None, refine_lr=None, prune=None, propose=None):
    """make_parse_score_logger's counterpart for scenes larger than the canvas (air.score_parse_tiled): `data` is an annotated dataset
    dict of SCENES (imgs [N, Hs, Ws], boxes [N, G, 4], instances [N, Hs, Ws] int8 -- data.create_multi_mnist with canvas_size = the
    scene's and return_annotations=True), walked in `num_batches` batches of `batch_size` scenes (None: the model's batch size).
    Prints / writes count accuracy, AP per threshold and mAP, foreground ARI, mean best overlap, and the totals of the merge's
    candidate states over the scenes scored (merge_kept, merge_not_owned, merge_duplicate, merge_overflow, merge_nonfinite)."""
    import torch
    from .tile import STATES
    kw = {} if thresholds is None else dict(thresholds=tuple(thresholds))
    tk = dict(stride=stride, iou_merge=iou_merge, refine=refine, refine_lr=refine_lr, prune=prune, propose=propose)

    def logger(itr=0, num_batches_to_eval=None, write=True):
        n = num_batches if num_batches_to_eval is None else num_batches_to_eval
        S = int(air.obs.shape[0]) if batch_size is None else int(batch_size)
        n = min(max(int(n), 1), int(data["imgs"].shape[0]) // S)
        if n < 1:
            raise ValueError("the annotated dataset holds fewer scenes than one batch of %d" % S)
        start = time.time()
        dev = air.obs.device
        states = torch.zeros(6, dtype=torch.int64, device=dev)
        scorer = None
        for i in range(n):
            sl = slice(i * S, (i + 1) * S)
            _, scorer = air.score_parse_tiled(torch.as_tensor(data["imgs"][sl], dtype=torch.float32).to(dev),
                                              torch.as_tensor(data["instances"][sl]), torch.as_tensor(data["boxes"][sl]),
                                              accumulate=i > 0, **kw, **tk)
            states += air.parsed_tiled["merge_counts"].sum(0)
        acc = scorer.summary()
        for k, v in zip(STATES[1:], states.tolist()[1:]):
            acc["merge_" + k] = v
        shown = ["count_acc", "map", "ap@%.2f" % scorer.thresholds_host[0], "fg_ari", "mean_best_overlap", "merge_kept",
                 "merge_not_owned", "merge_duplicate", "merge_overflow"]
        t = time.time() - start
        msg = 'Step {}, Data {} parse tiled score '.format(itr, name) + ', '.join('{} = {:.4f}'.format(k, acc[k]) for k in shown)
        if measure_time:
            msg += ', eval time = {:.4}s'.format(t)
        print(msg)
        if write and writer is not None:
            rec = dict(step=int(itr), data=name + "_parse_tiled_score", scene_size=list(data["imgs"].shape[1:]),
                       stride=None if stride is None else list(stride), **acc)
            writer.write(json.dumps(rec) + "\n"); writer.flush()
        return acc
    return logger


def make_track_fig(frames, result, max_frames=8, checkpoint_dir=None, global_step=None, n_samples=4):
    """The tracks of sequences (AIRonMNIST.track / track.SequenceTracker.track): one row per sequence, one panel per frame (the first
    `max_frames`), the frame with the attention box of every object that has a track, coloured by track id (rect_stn on `where`); an
    object without a track is drawn thin and white.  frames [S, F, H, W], result: the dict `track` returned; a stitcher's result
    (`track(stitch=...)`, track.TrackStitcher) is drawn with its STITCHED ids.  Saved as track_fig_<global_step>.png when a directory
    is given."""
    import os.path as osp
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    import torch
    host = lambda t: torch.as_tensor(t).detach().cpu().numpy()
    x, ids = host(frames), host(result["stitch_id"] if "stitch_id" in result else result["track_id"])
    where, n = host(result["where"]), host(result["num_objects"])
    S, F, H, W = x.shape
    T = ids.shape[0]
    rows, cols = min(n_samples, S), min(int(max_frames), F)
    inch = 1.5
    fig, axes = plt.subplots(rows, cols, figsize=(inch * cols * W / max(H, W), inch * rows * H / max(H, W)), squeeze=False)
    colours = plt.get_cmap('tab20')
    for s in range(rows):
        for f in range(cols):
            r, ax = s * F + f, axes[s][f]
            ax.imshow(x[s, f], cmap='gray', vmin=0, vmax=1)
            for j in range(min(T, max(int(n[r]), 0))):
                if ids[j, r] >= 0:
                    rect_stn(ax, W, H, where[j, r], colours(int(ids[j, r]) % 20), line_width=1)
                else:
                    rect_stn(ax, W, H, where[j, r], 'white', line_width=.3)
            ax.set_axis_off()
    if checkpoint_dir is not None:
        fig.savefig(osp.join(checkpoint_dir, 'track_fig_{}.png'.format(global_step)), dpi=300)
        plt.close(fig)
    return fig


def make_trajectory_fig(frames, result, max_frames=8, checkpoint_dir=None, global_step=None, n_samples=4, arrow_scale=3.0):
    """The trajectories of sequences (AIRonMNIST.track(smooth=...) / trajectory.TrajectorySmoother.result): one row per sequence, one
    panel per frame (the first `max_frames`), the frame with the SMOOTHED attention box of every row of the completed table, coloured
    by track id -- an observed row solid, a FILLED row (the track coasted over this frame) dashed -- and an arrow of `arrow_scale`
    frames of its velocity from the box centre; with a forecast horizon the predicted frames are appended, their forecast boxes
    dotted.  frames [S, F, H, W].  Saved as trajectory_fig_<global_step>.png when a directory is given."""
    import os.path as osp
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    import torch
    from .trajectory import FILLED
    host = lambda t: torch.as_tensor(t).detach().cpu().numpy()
    x, ids, boxes, state = host(frames), host(result["sm_id"]), host(result["sm_boxes"]), host(result["sm_state"])
    vel, n = host(result["sm_velocity"]), host(result["sm_count"])
    S, F, H, W = x.shape
    pred = host(result["frames_pred"]) if "frames_pred" in result else None
    Hz = 0 if pred is None else pred.shape[1]
    rows, shown = min(n_samples, S), min(int(max_frames), F)
    cols = shown + Hz
    inch = 1.5
    fig, axes = plt.subplots(rows, cols, figsize=(inch * cols * W / max(H, W), inch * rows * H / max(H, W)), squeeze=False)
    colours = plt.get_cmap('tab20')

    def draw(ax, box, colour, style):
        ax.add_patch(plt.Rectangle((box[0] - .5, box[1] - .5), box[2], box[3], fill=False, edgecolor=colour, linewidth=1, linestyle=style))

    for s in range(rows):
        for f in range(shown):
            r, ax = s * F + f, axes[s][f]
            ax.imshow(x[s, f], cmap='gray', vmin=0, vmax=1)
            for j in range(int(n[r])):
                colour = colours(int(ids[j, r]) % 20)
                draw(ax, boxes[j, r], colour, '--' if state[j, r] == FILLED else '-')
                cx, cy = boxes[j, r, 0] + boxes[j, r, 2] / 2 - .5, boxes[j, r, 1] + boxes[j, r, 3] / 2 - .5
                dx, dy = arrow_scale * vel[j, r, 0], arrow_scale * vel[j, r, 1]
                if dx or dy:
                    ax.annotate('', xy=(cx + dx, cy + dy), xytext=(cx, cy), arrowprops=dict(arrowstyle='->', color=colour, lw=.6))
            ax.set_axis_off()
        for k in range(Hz):
            c, ax = s * Hz + k, axes[s][shown + k]
            ax.imshow(pred[s, k], cmap='gray', vmin=0, vmax=1)
            fid, fbox = host(result["fc_id"]), host(result["fc_boxes"])
            for j in range(int(host(result["fc_count"])[c])):
                draw(ax, fbox[j, c], colours(int(fid[j, c]) % 20), ':')
            ax.set_title('+%d' % (k + 1), fontsize=5, pad=1)
            ax.set_axis_off()
    if checkpoint_dir is not None:
        fig.savefig(osp.join(checkpoint_dir, 'trajectory_fig_{}.png'.format(global_step)), dpi=300)
        plt.close(fig)
    return fig


def make_track_score_logger(air, data, num_batches, name, batch_size=None, writer=None, tau=0.5, measure_time=True, iou_gate=None,
                            appearance_weight=None, birth_score=None, max_age=None, refine=None, refine_lr=None, prune=None,
                            propose=None, temporal=None, smooth=None, matching=None, identity=False, motion=None, motion_gate=None,
                            hota=False, stitch=None, mots=False):
    """make_tiled_parse_score_logger's counterpart for sequences (air.score_track): `data` is an annotated dataset dict of SEQUENCES
    (imgs [N, F, H, W], boxes [N, F, G, 4], instances [N, F, H, W] int8 -- data.create_moving_mnist with return_annotations=True),
    walked in `num_batches` batches of `batch_size` sequences (None: the model's batch size).  Prints / writes the identity figures
    (MOTA, MOTP, identity switches, mostly tracked / lost), the per-frame detection figures of the same parses (count accuracy, mAP)
    and the totals of the association's object states (track_matched, track_born, track_unconfirmed, track_overflow,
    track_nonfinite) and the tracks issued.  temporal=P | (P, rounds): the frames' parses are repaired from their neighbour frames
    first (air.track's argument); temporal_kept then counts the objects that came from a neighbour.  smooth=True | dict: the tracks are
    also smoothed and gap-filled (trajectory.TrajectorySmoother) and the COMPLETED table is scored by the same kernel, side by side:
    smooth_mota, smooth_motp, smooth_id_switches, smooth_misses, smooth_false_positives, and the rows per state rows_observed,
    rows_filled.  matching="optimal": the optimal assignment of every frame instead of the greedy one (air.track's argument; the
    record names it).  identity=True: the IDF figures beside MOTA -- idf1, idp, idr, idtp, idfp, idfn (air_track_idf), and with smooth=
    smooth_idf1 of the completed table.  motion=True | dict: every track is matched against its predicted box (air.track's argument;
    the record holds the noise terms under `motion`).  motion_gate=True | D2 (with motion): the pairs are gated and ranked by their
    squared Mahalanobis distance (air.track's argument; the record holds the gate under `motion_gate`).  hota=True: HOTA beside MOTA
    -- hota, deta, assa, loca (air_track_hota; means over the 19 thresholds), and with smooth= smooth_hota of the completed table.
    stitch=True | MAX_GAP | dict (not with smooth=): the track fragments are joined across long occlusions (track.TrackStitcher,
    air.track's argument) and the STITCHED ids are scored beside the tracker's own on the same parses: stitch_mota,
    stitch_id_switches, stitch_links, with identity= stitch_idf1, with hota= stitch_hota and stitch_assa; the record holds max_gap and
    the gate under `stitch`.  mots=True: the tracks scored as MASKS beside MOTA -- motsa, smotsa, motsp (air_track_mots on the owner
    map and data["instances"]), with smooth= smooth_smotsa of the completed table, with stitch= stitch_smotsa of the stitched ids."""
    import torch
    from .track import STATES
    tk = dict(iou_gate=iou_gate, appearance_weight=appearance_weight, birth_score=birth_score, max_age=max_age, refine=refine,
              refine_lr=refine_lr, prune=prune, propose=propose, temporal=temporal)
    if smooth is not None:
        tk["smooth"] = smooth
    if matching is not None:
        tk["matching"] = matching
    if identity:
        tk["identity"] = True
    if motion is not None:
        tk["motion"] = motion
    if motion_gate is not None:
        tk["motion_gate"] = motion_gate
    if hota:
        tk["hota"] = True
    if stitch is not None:
        tk["stitch"] = stitch
    if mots:
        tk["mots"] = True

    def logger(itr=0, num_batches_to_eval=None, write=True):
        n = num_batches if num_batches_to_eval is None else num_batches_to_eval
        S = int(air.obs.shape[0]) if batch_size is None else int(batch_size)
        n = min(max(int(n), 1), int(data["imgs"].shape[0]) // S)
        if n < 1:
            raise ValueError("the annotated dataset holds fewer sequences than one batch of %d" % S)
        start = time.time()
        dev = air.obs.device
        states, issued = torch.zeros(6, dtype=torch.int64, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
        repaired = torch.zeros((), dtype=torch.int64, device=dev)
        table_rows = torch.zeros(3, dtype=torch.int64, device=dev)
        tracker = stitcher = None
        links = torch.zeros((), dtype=torch.int64, device=dev)
        for i in range(n):
            sl = slice(i * S, (i + 1) * S)
            _, tracker = air.score_track(torch.as_tensor(data["imgs"][sl], dtype=torch.float32).to(dev), torch.as_tensor(data["boxes"][sl]),
                                         tau=tau, accumulate=i > 0, gt_instances=torch.as_tensor(data["instances"][sl]), **tk)
            if stitch is not None:                                 # the stitcher was scored: the tracker's own ids beside it, same parses
                stitcher, tracker = tracker, tracker.tracker
                tracker.score(torch.as_tensor(data["boxes"][sl]), tau, i > 0, identity)
                if hota:
                    tracker.hota(torch.as_tensor(data["boxes"][sl]), i > 0)
                if mots:
                    tracker.mots(torch.as_tensor(data["instances"][sl]), int(data["boxes"].shape[-2]), i > 0)
                links += air.tracked["num_links"].sum()
            states += air.tracked["state_counts"].sum(0)
            issued += air.tracked["num_tracks"].sum()
            if temporal is not None:
                repaired += air.tracked["objects_temporal_kept"].sum()
            if smooth is not None:
                table_rows += air.tracked["sm_counts"].sum(0)
        acc = tracker.summary()
        det = air.track_scorer.summary()
        acc.update(count_acc=det["count_acc"], map=det["map"], frames=det["images"], objects_pred=det["objects_pred"],
                   tracks=int(issued.item()))
        if temporal is not None:
            acc["temporal_kept"] = int(repaired.item())
        for k, v in zip(STATES[1:], states.tolist()[1:]):
            acc["track_" + k] = v
        shown = ["mota", "motp", "id_switches", "mostly_tracked", "mostly_lost", "count_acc", "map", "tracks"]
        if smooth is not None:
            done = air.track_smoother.summary()
            for k in ("mota", "motp", "id_switches", "misses", "false_positives"):
                acc["smooth_" + k] = done[k]
            acc["rows_observed"], acc["rows_filled"] = (int(v) for v in table_rows.tolist()[1:])
            shown += ["smooth_mota", "smooth_motp", "rows_filled"]
        if identity:
            idf = tracker.identity_summary()
            acc.update({k: idf[k] for k in ("idf1", "idp", "idr", "idtp", "idfp", "idfn")})
            shown[2:2] = ["idf1", "idp", "idr"]
            if smooth is not None:
                acc["smooth_idf1"] = air.track_smoother.identity_summary()["idf1"]
                shown += ["smooth_idf1"]
        if hota:
            fig = tracker.hota_summary()
            acc.update({k: fig[k] for k in ("hota", "deta", "assa", "loca")})
            shown[2:2] = ["hota", "deta", "assa", "loca"]
            if smooth is not None:
                acc["smooth_hota"] = air.track_smoother.hota_summary()["hota"]
                shown += ["smooth_hota"]
        if mots:
            fig = tracker.mots_summary()
            acc.update({k: fig[k] for k in ("motsa", "smotsa", "motsp")})
            shown[2:2] = ["motsa", "smotsa", "motsp"]
            if smooth is not None:
                acc["smooth_smotsa"] = air.track_smoother.mots_summary()["smotsa"]
                shown += ["smooth_smotsa"]
        if stitch is not None:
            joined = stitcher.summary()
            acc.update(stitch_mota=joined["mota"], stitch_id_switches=joined["id_switches"], stitch_links=int(links.item()))
            shown += ["stitch_mota", "stitch_id_switches", "stitch_links"]
            if identity:
                acc["stitch_idf1"] = stitcher.identity_summary()["idf1"]
                shown += ["stitch_idf1"]
            if hota:
                fig = stitcher.hota_summary()
                acc.update(stitch_hota=fig["hota"], stitch_assa=fig["assa"])
                shown += ["stitch_hota", "stitch_assa"]
            if mots:
                acc["stitch_smotsa"] = stitcher.mots_summary()["smotsa"]
                shown += ["stitch_smotsa"]
        t = time.time() - start
        msg = 'Step {}, Data {} track score '.format(itr, name) + ', '.join('{} = {:.4f}'.format(k, acc[k]) for k in shown)
        if measure_time:
            msg += ', eval time = {:.4}s'.format(t)
        print(msg)
        if write and writer is not None:
            rec = dict(step=int(itr), data=name + "_track_score", n_frames=int(data["imgs"].shape[1]), tau=float(tau),
                       iou_gate=tracker.iou_gate, appearance_weight=tracker.appearance_weight, birth_score=tracker.birth_score,
                       max_age=tracker.max_age, **acc)
            if matching is not None:
                rec["matching"] = tracker.matching
            if motion is not None:
                rec["motion"] = {k: list(v) if isinstance(v, tuple) else v for k, v in tracker.motion.items()}
            if motion_gate is not None:
                rec["motion_gate"] = tracker.motion_gate
            if stitch is not None:
                rec["stitch"] = dict(max_gap=stitcher.max_gap, gate=stitcher.gate, appearance_weight=stitcher.appearance_weight)
            writer.write(json.dumps(rec) + "\n"); writer.flush()
        return acc
    return logger


def make_track_stream_logger(air, data, num_batches, name, chunk_frames, batch_size=None, writer=None, tau=0.5, measure_time=True,
                             smooth=None, **stream_args):
    """make_track_score_logger's counterpart for STREAMS (air.track_stream, track.StreamTracker): the sequences of `data` (imgs
    [N, F, H, W], boxes [N, F, G, 4]) are fed in chunks of `chunk_frames` frames, the last chunk ragged (`valid`), every batch of
    `batch_size` sequences as a stream of its own (reset between batches), each chunk scored against its rows of the ground truth.
    Prints / writes the tracker's summary() summed over the batches -- the counts add up; the rates come from track.mot_summary on the
    sums -- and the tracks issued.  `stream_args` are AIRonMNIST.stream_tracker's.  smooth=True | dict(lag=, horizon=, ...): the stream
    goes through a trajectory.StreamSmoother (air.stream_smoother) and the EMITTED frames are scored instead -- fixed-lag smoothed and
    gap-filled, `lag` frames late, each against the ground truth of its own global frame (emit_frame is read back per chunk); the last
    `lag` frames of a sequence are never emitted and are not scored.  Logged as <name>_track_stream_smooth."""
    import numpy as np
    import torch
    from .track import COUNTS, mot_summary

    def logger(itr=0, num_batches_to_eval=None, write=True):
        n = num_batches if num_batches_to_eval is None else num_batches_to_eval
        S = int(air.obs.shape[0]) if batch_size is None else int(batch_size)
        n = min(max(int(n), 1), int(data["imgs"].shape[0]) // S)
        if n < 1:
            raise ValueError("the annotated dataset holds fewer sequences than one batch of %d" % S)
        start = time.time()
        dev = air.obs.device
        F, C = int(data["imgs"].shape[1]), int(chunk_frames)
        G = int(data["boxes"].shape[-2])
        totals, sum_iou, issued = np.zeros(8, np.int64), 0.0, 0
        for i in range(n):
            sl = slice(i * S, (i + 1) * S)
            imgs, boxes = np.asarray(data["imgs"][sl], np.float32), np.asarray(data["boxes"][sl], np.float32)
            smoother = None if smooth is None else air.stream_smoother(S, C, smooth, **stream_args)
            tracker = air.stream_tracker(S, C, **stream_args) if smoother is None else smoother.tracker
            if smoother is None:
                tracker.score_reset()
            for at in range(0, F, C):
                v = min(C, F - at)
                frames, gt = np.zeros((S, C) + imgs.shape[2:], np.float32), np.zeros((S, C, G, 4), np.float32)
                frames[:, :v], gt[:, :v] = imgs[:, at:at + v], boxes[:, at:at + v]
                out = air.track_stream(torch.from_numpy(frames).to(dev), np.full(S, v, np.int64), reset=at == 0, smooth=smooth,
                                       **stream_args)
                if smoother is None:
                    scores = tracker.score(torch.from_numpy(gt), tau)
                else:                                              # the ground truth of the frames this push emitted
                    emit = out["emit_frame"].cpu().numpy()
                    gt[:] = 0
                    for s_, e_ in zip(*np.nonzero(emit >= 0)):
                        gt[s_, e_] = boxes[s_, emit[s_, e_]]
                    scores = smoother.score(torch.from_numpy(gt), tau)
            tracker.synchronize()
            totals += scores["seq_counts"].sum(0, dtype=torch.int64).cpu().numpy()
            sum_iou += float(scores["seq_iou"].sum().item())
            issued += int(tracker.state["seq"][:, 1].sum().item())
        acc = mot_summary(totals, sum_iou)
        acc["tracks"] = issued
        shown = ["mota", "motp", "id_switches", "mostly_tracked", "mostly_lost", "tracks"]
        t = time.time() - start
        msg = 'Step {}, Data {} track stream '.format(itr, name) + ', '.join('{} = {:.4f}'.format(k, acc[k]) for k in shown)
        if measure_time:
            msg += ', eval time = {:.4}s'.format(t)
        print(msg)
        if write and writer is not None:
            rec = dict(step=int(itr), data=name + ("_track_stream" if smooth is None else "_track_stream_smooth"), n_frames=F,
                       chunk_frames=C, tau=float(tau), iou_gate=tracker.iou_gate, appearance_weight=tracker.appearance_weight,
                       birth_score=tracker.birth_score, max_age=tracker.max_age, matching=tracker.matching, **acc)
            if smooth is not None:
                rec.update(lag=smoother.lag, horizon=smoother.horizon)
            writer.write(json.dumps(rec) + "\n"); writer.flush()
        return acc
    return logger


def gradient_summaries(named_grads, named_vars, norm=True, ratio=True, histogram=False, bins=30):
    """evaluation.py:221-248: the global norm of the gradient, per variable mean(|g| / (|v| + 1e-8)) (log_ratio,
    evaluation.py:169-180) and -- histogram=True, the reference's default -- a histogram of every gradient tensor, the content of its
    `tf.summary.histogram('grad_hist/<name>', g)` as plain data: {'counts': [...], 'edges': [...]} over `bins` equal-width bins between
    the tensor's min and max (TensorBoard's own compression of the same values is a display artefact).  `named_grads` / `named_vars`:
    name -> tensor (AIREngine.named_grads() / .params; on the engine the gradients are those of the last update and the variables the
    ones it produced).  Returns {'grad_norm': float, 'grad_ratio/<name>': float, 'grad_hist/<name>': dict}.  Off by default here
    because the script logs JSON lines, not event files: scripts/multi_mnist.py --grad-histograms switches it on."""
    import torch
    out = {}
    if norm:
        out['grad_norm'] = float(torch.sqrt(sum((g.double() ** 2).sum() for g in named_grads.values())))
    for k, g in named_grads.items():
        if ratio:
            out['grad_ratio/' + k] = float((g.abs() / (named_vars[k].abs() + 1e-8)).mean())
        if histogram:
            gf = g.detach().float().reshape(-1)
            fin = gf[torch.isfinite(gf)]
            lo, hi = (float(fin.min()), float(fin.max())) if fin.numel() else (0.0, 0.0)
            if hi <= lo:
                hi = lo + 1e-12
            counts = torch.histc(fin, bins=bins, min=lo, max=hi) if fin.numel() else torch.zeros(bins)
            out['grad_hist/' + k] = {'counts': [int(c) for c in counts.tolist()],
                                     'edges': [lo + (hi - lo) * i / bins for i in range(bins + 1)],
                                     'non_finite': int(gf.numel() - fin.numel())}
    return out


def step_summaries(air, histogram=False):
    """The scalars the reference registers with tf.summary.scalar and writes every 1000 iterations (multi_mnist.py:138-140;
    model.py:152,185,213,244-257,323-371), read from the engine after a train step: the objective's terms on the batch just
    trained on + the gradient summaries of that update."""
    eng = air._engine
    o = eng.outputs()
    pick = ["rec_loss", "kl_num_steps", "kl_what", "kl_where", "prior_loss", "loss", "opt_loss"]
    if eng.cfg.use_reinforce:
        pick += ["imp_weight_mean", "imp_weight_var", "reinforce_loss", "baseline_loss"]
    out = {('rec' if k == 'rec_loss' else 'prior' if k == 'prior_loss' else k): _scalar(o[k]) for k in pick}
    out['num_step'] = _scalar(o["num_step_per_sample"].mean())
    out.update(gradient_summaries(eng.named_grads(), eng.params, histogram=histogram))
    return out


def _scalar(v):
    return float(v.item()) if hasattr(v, "item") else float(v)


def logged_exprs(air):
    """The scalar set of evaluation.py:69-92, as name -> callable(air) (eager mode: attributes are refreshed per pass)."""
    exprs = {
        'loss': lambda a: a.loss.value,
        'rec_loss': lambda a: a.rec_loss,
        'num_step_acc': lambda a: a.num_step_accuracy,
        'num_step': lambda a: a.num_step,
    }
    if air.use_prior:
        exprs['prior_loss'] = lambda a: a.prior_loss.value
        if air.num_steps_prior is not None:
            exprs['kl_num_steps'] = lambda a: a.kl_num_steps
        if air.what_prior is not None:
            exprs['kl_what'] = lambda a: a.kl_what
            exprs['kl_where'] = lambda a: a.kl_where
    if air.use_reinforce:
        if air.baseline is not None:
            exprs['baseline_loss'] = lambda a: a.baseline_loss
        exprs['reinforce_loss'] = lambda a: a.reinforce_loss
        exprs['imp_weight'] = lambda a: a.importance_weight.mean()
    return exprs


def make_expr_logger(air, data_fn, num_batches, expr_dict, name, writer=None, measure_time=True):
    """evaluation.py:112-166: average `expr_dict` over `num_batches` evaluation passes on batches from `data_fn`."""
    def logger(itr=0, num_batches_to_eval=None, write=True):
        n = num_batches if num_batches_to_eval is None else num_batches_to_eval
        n = max(int(n), 1)
        acc = {k: 0. for k in expr_dict}
        start = time.time()
        for _ in range(n):
            obs, nums = data_fn()
            air.evaluate(obs, nums)
            for k, fn in expr_dict.items():
                acc[k] += _scalar(fn(air))
        acc = {k: v / n for k, v in acc.items()}
        t = time.time() - start
        msg = 'Step {}, Data {} '.format(itr, name) + ', '.join('{} = {:.4f}'.format(k, v) for k, v in acc.items())
        if measure_time:
            msg += ', eval time = {:.4}s'.format(t)
        print(msg)
        if write and writer is not None:
            writer.write(json.dumps(dict(step=int(itr), data=name, **acc)) + "\n"); writer.flush()
        return acc
    return logger


def make_iw_logger(air, data_fn, num_batches, particles, name, writer=None, measure_time=True):
    """The K-particle importance-weighted bound, the ELBO of the same particles, the effective sample size and the count
    accuracy of the self-normalised posterior, averaged over `num_batches` batches from `data_fn` (air.evaluate_iw; the sums
    live on the device in float64 and are read once).  Prints / writes one line like make_expr_logger."""
    def logger(itr=0, num_batches_to_eval=None, write=True):
        n = num_batches if num_batches_to_eval is None else num_batches_to_eval
        n = max(int(n), 1)
        start = time.time()
        ev = air.iw_evaluator(particles)
        ev.reset()
        for _ in range(n):
            obs, nums = data_fn()
            air.evaluate_iw(obs, nums, particles=particles)
        acc = ev.totals()
        t = time.time() - start
        msg = 'Step {}, Data {} IW({}) '.format(itr, name, particles) + ', '.join('{} = {:.4f}'.format(k, v) for k, v in acc.items())
        if measure_time:
            msg += ', eval time = {:.4}s'.format(t)
        print(msg)
        if write and writer is not None:
            writer.write(json.dumps(dict(step=int(itr), data=name + "_iw", particles=int(particles), **acc)) + "\n"); writer.flush()
        return acc
    return logger


def make_logger(air, train_data_fn, train_batches, test_data_fn, test_batches, writer=None):
    """evaluation.py:68-109.  (The reference divides the batch counts by batch_size a second time, evaluation.py:94,100
    -- SURVEY B-8; here `*_batches` is simply the number of batches to average over.)"""
    exprs = logged_exprs(air)
    train_log = make_expr_logger(air, train_data_fn, train_batches, exprs, 'train', writer)
    test_log = make_expr_logger(air, test_data_fn, test_batches, exprs, 'test', writer)

    def log(train_itr):
        a = train_log(train_itr)
        b = test_log(train_itr)
        print()
        return a, b
    return log
