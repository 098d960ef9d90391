#!/usr/bin/env python
"""Counterpart of the reference's training script (attend_infer_repeat/scripts/multi_mnist.py:24-147): same
hyper-parameters, same loop structure (train / periodic log / periodic figure + checkpoint), on the MI355X engine.

Data: `--data-dir` with mnist_train.pickle / mnist_validation.pickle (Python-3 pickles with the reference's layout) if
present; otherwise a synthetic multi-MNIST-shaped dataset (no network here, so no MNIST download).  The dataset lives
in HBM and batches are index gathers (data.DeviceFeeder) instead of a tf.py_func host round trip per step.
"""
import argparse
import json
import os
import os.path as osp
import sys
import time

ROOT = osp.dirname(osp.dirname(osp.dirname(osp.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from attend_infer_repeat_amd.data import DeviceFeeder, load_data, procedural_multi_mnist, synthetic_dataset  # noqa: E402
from attend_infer_repeat_amd.evaluation import (make_fig, make_iw_logger, make_logger, make_parse_fig, make_parse_logger, make_parse_score_logger,  # noqa: E402
                                                make_prior_fig, step_summaries)
from attend_infer_repeat_amd.mnist_model import AIRonMNIST  # noqa: E402
from attend_infer_repeat_amd.utils import AttrDict  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=int(3e5))            # multi_mnist.py:134
    ap.add_argument("--log-every", type=int, default=10000)           # :142
    ap.add_argument("--save-every", type=int, default=5000)           # :145
    ap.add_argument("--results-dir", default="../results")
    ap.add_argument("--run-name", default="multi_mnist")
    ap.add_argument("--data-dir", default="data")
    ap.add_argument("--synthetic-samples", type=int, default=60000)
    ap.add_argument("--eval-batches", type=int, default=10)
    ap.add_argument("--figures", action="store_true")
    ap.add_argument("--summary-every", type=int, default=1000)        # multi_mnist.py:138-140
    ap.add_argument("--glyphs", action="store_true",
                    help="no multi-MNIST pickles: synthesise the dataset with the reference's generator (data.create_multi_mnist) "
                         "from procedural digit templates instead of stroke blobs")
    ap.add_argument("--learning-rate", type=float, default=1e-4)
    ap.add_argument("--check-every", type=int, default=0,
                    help="diagnostics (read-only: does not touch the noise stream): every N updates from --check-from on, write the "
                         "extreme values of the latents' scales, of the parameters, gradients and RMSProp slots to log.jsonl")
    ap.add_argument("--check-from", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-feeder", action="store_true",
                    help="draw every training batch inside the captured step from the HBM-resident training set (engine "
                         "attach_dataset): no host work between updates")
    ap.add_argument("--guard-degenerate", type=float, default=0.0,
                    help="stability switch, default off (= the reference's arithmetic): floor of both Gaussian heads' scale and "
                         "minimum |scale component| of the sampled `where` (AIRonMNIST(guard_degenerate=...); e.g. 1e-6)")
    ap.add_argument("--resume", default=None,
                    help="checkpoint written by this script (model_<iter>.pt): restores parameters, the RMSProp slots, "
                         "the step counter, the learning rate, the Philox noise state and the feeders' positions")
    ap.add_argument("--init-from-tf-ckpt", default=None, metavar="PREFIX",
                    help="prefix of a checkpoint the reference's tf.train.Saver wrote (e.g. ../results/multi_mnist/model.ckpt-175000): "
                         "the model / baseline variables become the initial parameters, its RMSProp slots (where the file holds them) the "
                         "optimiser state and its global_step the step counter (tf_checkpoint.py: format and names unvalidated without TensorFlow)")
    ap.add_argument("--grad-histograms", action="store_true",
                    help="add the per-variable gradient histograms of evaluation.gradient_summaries(histogram=True) (the reference's default, "
                         "evaluation.py:221-248) to the 1000-iteration summaries in log.jsonl")
    ap.add_argument("--iw-particles", type=int, default=0, metavar="K",
                    help="K > 0: at every --log-every also print / write the K-particle importance-weighted bound, the ELBO of the same "
                         "particles, the effective sample size and the count accuracy of the self-normalised posterior on the validation "
                         "batches (evaluation.make_iw_logger); 0 = off")
    ap.add_argument("--iw-train", type=int, default=None, metavar="K",
                    help="K >= 2: train on the K-particle importance-weighted bound (AIRonMNIST.train_step(iw_samples=K): IWAE weights "
                         "for the continuous latents, VIMCO's leave-one-out signal for the object count, no baseline) on the generic "
                         "autograd path -- the fused engine is not used; iw_bound, iw_ess and iw_degenerate go into the 1000-iteration "
                         "summaries.  Not with --decay-rate or the options that need the engine")
    ap.add_argument("--iw-objective", choices=("vimco", "rws"), default=None,
                    help="with --iw-train K: the gradient estimator.  vimco (the default): IWAE weights and VIMCO's leave-one-out signal; "
                         "rws: the wake-phase update of reweighted wake-sleep -- the particles are fixed values, the decoder follows "
                         "sum_k w_k grad log p(x, z_k), the inference network sum_k w_k grad log q(z_k | x)")
    ap.add_argument("--decay-rate", type=float, default=None, metavar="D",
                    help="train_step's decay_rate: normalise the NVIL importance weight by moving averages with decay D (the reference "
                         "script leaves it off)")
    ap.add_argument("--prior-samples", type=int, default=0, metavar="N",
                    help="N > 0: at every --log-every draw N scenes from the generative model on the device (AIRonMNIST.sample_scenes, the "
                         "model's own count prior) and write the histogram of the generated object counts to log.jsonl; with --figures also "
                         "prior_fig_<iter>.png (evaluation.make_prior_fig, uniform counts); 0 = off")
    ap.add_argument("--parse-eval", action="store_true",
                    help="at every --log-every also print / write the deterministic parse of the validation batches (AIRonMNIST.parse, "
                         "evaluation.make_parse_logger): the accuracy of the MAP object count, the mean q(n) at the mode and the mean number "
                         "of objects per image; with --figures also parse_fig_<iter>.png (evaluation.make_parse_fig)")
    ap.add_argument("--parse-score", action="store_true",
                    help="at every --log-every also score the deterministic parse of the validation set against its annotations on the "
                         "device (AIRonMNIST.score_parse, evaluation.make_parse_score_logger): count accuracy, precision / recall / F1 / AP "
                         "over box-IoU thresholds, foreground ARI and mean best overlap of the instance masks.  Needs annotated data: "
                         "--glyphs, or pickles written by create_dataset.py --annotations")
    ap.add_argument("--parse-particles", type=int, default=0, metavar="K",
                    help="K > 0: --parse-eval and --parse-score parse with K posterior particles per image and keep the best one "
                         "(AIRonMNIST.parse(particles=K), particle_parse.ParticleParser) instead of the parse at the mode; the log record "
                         "names K and the criterion; 0 = the deterministic parse")
    ap.add_argument("--parse-select", default="joint", choices=("joint", "weight"),
                    help="with --parse-particles: the particle kept per image -- 'joint' = the largest log p(x, z), 'weight' = the largest "
                         "importance weight log p(x, z) - log q(z | x)")
    ap.add_argument("--parse-refine", type=int, default=None, metavar="N",
                    help="--parse-eval and --parse-score refine the parse by N gradient-ascent iterations on log p(x, z) in the continuous "
                         "latents (AIRonMNIST.parse(refine=N), refine.ParseRefiner) behind the parse at the mode or the best of "
                         "--parse-particles; the log record names N and adds objective_gain and refine_moved; N = 0 evaluates the start "
                         "parse's objective only")
    ap.add_argument("--parse-prune", choices=("present", "all"), default=None,
                    help="--parse-eval and --parse-score search the subsets of the computed steps for the largest log p(x, z) "
                         "(AIRonMNIST.parse(prune=...), prune.ParsePruner) behind the parse, its particles and its refinement: "
                         "\"present\" can only remove objects, \"all\" may also switch on a step the presence chain left out; the log "
                         "record names the mode and adds count_changed, objects_dropped, objects_added and objective_gain")
    ap.add_argument("--parse-propose", default=None, metavar="P[,ROUNDS]",
                    help="--parse-eval and --parse-score propose P missed objects per round from the residual image behind the parse, its "
                         "particles and its refinement, and search the pool of max_steps + P <= 6 rows for the largest log p(x, z) "
                         "(AIRonMNIST.parse(propose=...), propose.ParseProposer), ROUNDS times (default 1); not together with "
                         "--parse-prune; the log record names the spec and adds objects_added_from_residual, count_changed and "
                         "objective_gain")
    ap.add_argument("--parse-refine-lr", default=None, metavar="A,B",
                    help="with --parse-refine: the Adam learning rates of the `what` and the `where` latents (default: refine.DEFAULT_LR)")
    ap.add_argument("--parse-tiled", default=None, metavar="HSxWS[:STRIDE]",
                    help="at every --log-every also parse and score held-out SCENES of HS x WS pixels, larger than the model's canvas, "
                         "in overlapping windows merged on the device (AIRonMNIST.score_parse_tiled, tile.TiledSceneParser, "
                         "evaluation.make_tiled_parse_score_logger): count accuracy, AP / mAP, foreground ARI and the totals of the "
                         "merge's candidate states.  STRIDE: one number or SYxSX (default: half the canvas).  The scenes are built "
                         "from procedural digit templates by the reference's generator with annotations; --parse-refine, "
                         "--parse-prune and --parse-propose apply to every window")
    ap.add_argument("--parse-tiled-objects", type=int, default=4, metavar="N",
                    help="with --parse-tiled: a scene holds 0..N digits (N <= 8, the ground-truth slots of the scorer)")
    ap.add_argument("--track-eval", default=None, metavar="F[:SPEED]",
                    help="at every --log-every also track held-out SEQUENCES of F frames on the model's canvas and score the identities "
                         "on the device (AIRonMNIST.score_track, track.SequenceTracker, evaluation.make_track_score_logger): MOTA, MOTP, "
                         "identity switches, mostly tracked / lost, next to the per-frame count accuracy and mAP.  The sequences are "
                         "procedural digits that move in straight lines at up to SPEED pixels per frame (default 3) and reflect off "
                         "the canvas edges (data.procedural_moving_mnist, with births and deaths); --parse-refine, --parse-prune and "
                         "--parse-propose apply to every frame")
    ap.add_argument("--track-temporal", default=None, metavar="P[,ROUNDS]",
                    help="with --track-eval: before the association, propose to every frame up to P objects its parse missed from the "
                         "parses of the frames before and after it, ROUNDS times (default 1; temporal.TemporalProposer: the exact "
                         "subset search of --parse-prune over the frame's rows and its neighbours' rows, no network evaluation); "
                         "max_steps + P <= 6")
    ap.add_argument("--track-smooth", nargs="?", const="", default=None, metavar="QS,QC,R",
                    help="with --track-eval: smooth and gap-fill the tracks on the device (trajectory.TrajectorySmoother: a constant-rate "
                         "Kalman filter and a backward pass per track) and score the completed table next to the raw one.  QS,QC,R: the "
                         "process noise of the shifts and of the scales and the measurement noise, in `where` units (default "
                         "1e-4,1e-4,4e-4: provisional, unmeasured on a trained model)")
    ap.add_argument("--track-fit-noise", nargs="?", const=0, default=None, type=int, metavar="ZOOM",
                    help="with --track-eval: fit the trajectory smoother's noise terms to the tracks of the same sequences by maximum "
                         "likelihood on the device (AIRonMNIST.fit_track_noise: no ground truth is read) and log them as "
                         "<name>_track_noise_fit with loglik / n_innovations and the same figure at the current defaults; ZOOM > 0 "
                         "refines the grid ZOOM times around the best cell (needs --eval-batches 1)")
    ap.add_argument("--track-motion", nargs="?", const="", default=None, metavar="QS,QC,R,VV",
                    help="with --track-eval: match every track against where a per-track Kalman filter predicts it to be, not against "
                         "its last box (track.SequenceTracker's motion): no value = the default noise terms, QS,QC,R,VV = process noise "
                         "of shifts and scales, measurement noise, prior variance of the rate.  With --track-fit-noise the identity "
                         "figures are also logged with motion at the defaults and at the fitted terms (<name>_motion_defaults, "
                         "<name>_motion_fit); does not apply to --track-stream (out of scope on a stream)")
    ap.add_argument("--track-motion-gate", nargs="?", const="", default=None, metavar="D2",
                    help="with --track-motion: gate every (track, object) pair by its squared Mahalanobis distance from the filter's "
                         "predicted state, D2 at most, and rank by it instead of the IoU (track.SequenceTracker's motion_gate): no value = "
                         "13.2767, the 0.99 quantile of chi-squared with 4 degrees of freedom (provisional).  With --track-fit-noise the "
                         "<name>_motion_defaults / <name>_motion_fit figures are those under the gate")
    ap.add_argument("--track-matching", choices=("greedy", "optimal"), default=None,
                    help="with --track-eval: how a frame's objects are matched to the live tracks (track.SequenceTracker's matching): "
                         "greedy (the default) or the optimal assignment of the whole frame (Hungarian, air_track_associate_optimal)")
    ap.add_argument("--track-identity", action="store_true",
                    help="with --track-eval: also report IDF1, IDP and IDR (air_track_idf: how long each ground-truth object keeps one "
                         "identity) beside MOTA")
    ap.add_argument("--track-hota", action="store_true",
                    help="with --track-eval: also report HOTA, DetA, AssA and LocA (air_track_hota: how well objects are found and how "
                         "well the matched detections are kept in one identity, over 19 localisation thresholds) beside MOTA; not with "
                         "--track-stream (HOTA is out of scope on a stream)")
    ap.add_argument("--track-mots", action="store_true",
                    help="with --track-eval: also report MOTSA, sMOTSA and MOTSP (air_track_mots: the tracks scored as MASKS -- the "
                         "owner map against the instance maps, mask IoU > 1/2 decided in integers) beside MOTA; not with --track-stream "
                         "(MOTS is out of scope on a stream)")
    ap.add_argument("--track-stitch", nargs="?", const="", default=None, metavar="MAX_GAP[,D2]",
                    help="with --track-eval: join track fragments across occlusions longer than max_age (track.TrackStitcher: a track "
                         "that ended is linked to one that began at most MAX_GAP frames later when its Kalman filter predicts the later "
                         "one's first sighting within the squared Mahalanobis distance D2 and their what codes agree, one optimal "
                         "assignment per sequence) and log the MOT, identity and HOTA figures of the stitched ids beside the tracker's "
                         "own (stitch_mota, stitch_idf1, stitch_hota, ...): no value = MAX_GAP 8 and D2 13.2767 (both provisional); not "
                         "with --track-stream or --track-smooth (out of scope there)")
    ap.add_argument("--track-stream", type=int, default=None, metavar="CHUNK",
                    help="with --track-eval: also run the same sequences through a STREAM in chunks of CHUNK frames (the last chunk "
                         "ragged; AIRonMNIST.track_stream, track.StreamTracker: the track table carried on the device between the chunks) "
                         "and log its summary() as <name>_track_stream; --track-matching and --track-temporal apply, --track-smooth and "
                         "--track-identity do not (--track-stream-smooth is the stream's smoother; IDF1 is out of scope on a stream)")
    ap.add_argument("--track-stream-smooth", type=str, default=None, metavar="LAG[,HZ]",
                    help="with --track-stream: also run the stream through a trajectory.StreamSmoother with lag LAG (max_age..16) and "
                         "horizon HZ (0..16, default 0) and log the score of the EMITTED frames (fixed-lag smoothed, gap-filled, LAG "
                         "frames late) as <name>_track_stream_smooth; the lag and the noise terms are provisional")
    ap.add_argument("--track-predict", type=int, default=None, metavar="HZ",
                    help="with --track-eval: also extrapolate the live tracks HZ frames (1..16) past every sequence and render the "
                         "predicted frames (AIRonMNIST.predict_frames' forecast table; implies --track-smooth)")
    ap.add_argument("--tf-name-map", default=None, metavar="JSON",
                    help="with --init-from-tf-ckpt: a JSON file {engine parameter name: checkpoint variable name} that replaces the shape-based "
                         "matcher (tf_checkpoint.default_name_map) when it stops or guesses wrong")
    args = ap.parse_args(argv)
    if args.iw_objective is not None and args.iw_train is None:
        ap.error("--iw-objective chooses the estimator of --iw-train K and needs it")
    if args.iw_train is not None:
        from attend_infer_repeat_amd.iw_train import NO_DECAY_RATE, check_iw_samples
        try:
            check_iw_samples(args.iw_train)
        except ValueError as e:
            ap.error("--iw-train: %s" % e)
        if args.decay_rate is not None:
            ap.error("--iw-train does not go with --decay-rate: %s" % NO_DECAY_RATE)
        needs_engine = [flag for flag, on in (
            ("--device-feeder", args.device_feeder), ("--resume", args.resume), ("--init-from-tf-ckpt", args.init_from_tf_ckpt),
            ("--check-every", args.check_every), ("--iw-particles", args.iw_particles > 0), ("--prior-samples", args.prior_samples > 0),
            ("--parse-eval", args.parse_eval), ("--parse-score", args.parse_score), ("--parse-tiled", args.parse_tiled),
            ("--track-eval", args.track_eval), ("--grad-histograms", args.grad_histograms)) if on]
        if needs_engine:
            ap.error("--iw-train runs on the generic autograd path; %s need(s) the fused engine" % ", ".join(needs_engine))
    refine_kw = {}
    if args.parse_refine_lr is not None and args.parse_refine is None:
        ap.error("--parse-refine-lr goes with --parse-refine")
    if args.parse_refine is not None:
        if args.parse_refine < 0:
            ap.error("--parse-refine needs N >= 0")
        refine_kw["refine"] = args.parse_refine
        if args.parse_refine_lr is not None:
            try:
                lr = tuple(float(v) for v in args.parse_refine_lr.split(","))
            except ValueError:
                lr = ()
            if len(lr) != 2 or min(lr) < 0:
                ap.error("--parse-refine-lr needs two learning rates >= 0 as A,B, got %r" % args.parse_refine_lr)
            refine_kw["refine_lr"] = lr
    if args.parse_prune is not None:
        refine_kw["prune"] = args.parse_prune
    if args.parse_propose is not None:
        if args.parse_prune is not None:
            ap.error("--parse-propose and --parse-prune exclude each other: the search over the pool already contains --parse-prune all")
        try:
            spec = tuple(int(v) for v in args.parse_propose.split(","))
        except ValueError:
            spec = ()
        if len(spec) not in (1, 2) or min(spec) < 1:
            ap.error("--parse-propose needs P >= 1 or P,ROUNDS with ROUNDS >= 1, got %r" % args.parse_propose)
        refine_kw["propose"] = spec[0] if len(spec) == 1 else spec

    tiled = None
    if args.parse_tiled is not None:
        try:
            size, _, stride = args.parse_tiled.partition(":")
            scene = tuple(int(v) for v in size.lower().split("x"))
            stride = tuple(int(v) for v in stride.lower().split("x")) if stride else None
            if len(scene) != 2 or (stride is not None and len(stride) not in (1, 2)):
                raise ValueError
        except ValueError:
            ap.error("--parse-tiled needs HSxWS or HSxWS:STRIDE (STRIDE: a number or SYxSX), got %r" % args.parse_tiled)
        if not 1 <= args.parse_tiled_objects <= 8:
            ap.error("--parse-tiled-objects needs 1 <= N <= 8")
        if args.parse_particles > 0:
            ap.error("--parse-tiled does not go with --parse-particles: particle providers are out of scope for tiling")
        tiled = dict(scene=scene, stride=None if stride is None else (stride * 2)[:2])

    track_eval = None
    if args.track_eval is not None:
        try:
            frames, _, top = args.track_eval.partition(":")
            track_eval = dict(frames=int(frames), speed=float(top) if top else 3.0)
        except ValueError:
            ap.error("--track-eval needs F or F:SPEED (F: frames per sequence, SPEED: pixels per frame), got %r" % args.track_eval)
        if not 1 <= track_eval["frames"] <= 32767 // 3:
            ap.error("--track-eval needs 1 <= F <= %d (F * max_steps track ids must fit int16)" % (32767 // 3))
        if not track_eval["speed"] >= 0.0 or track_eval["speed"] == float("inf"):
            ap.error("--track-eval needs a finite SPEED >= 0, got %r" % args.track_eval)
        if args.parse_particles > 0:
            ap.error("--track-eval does not go with --parse-particles: particle providers are out of scope for tracking")

    track_temporal = None
    if args.track_temporal is not None:
        try:
            spec = tuple(int(v) for v in args.track_temporal.split(","))
        except ValueError:
            spec = ()
        if len(spec) not in (1, 2) or min(spec) < 1:
            ap.error("--track-temporal needs P >= 1 or P,ROUNDS with ROUNDS >= 1, got %r" % args.track_temporal)
        if track_eval is None:
            ap.error("--track-temporal goes with --track-eval")
        track_temporal = spec[0] if len(spec) == 1 else spec

    if (args.track_matching is not None or args.track_identity) and track_eval is None:
        ap.error("--track-matching and --track-identity go with --track-eval")
    if args.track_hota and track_eval is None:
        ap.error("--track-hota goes with --track-eval")
    if args.track_hota and args.track_stream is not None:
        ap.error("--track-hota does not go with --track-stream (HOTA is out of scope on a stream)")
    if args.track_mots and track_eval is None:
        ap.error("--track-mots goes with --track-eval")
    if args.track_mots and args.track_stream is not None:
        ap.error("--track-mots does not go with --track-stream (MOTS is out of scope on a stream)")
    track_stitch = None
    if args.track_stitch is not None:
        if track_eval is None:
            ap.error("--track-stitch goes with --track-eval")
        if args.track_stream is not None:
            ap.error("--track-stitch does not go with --track-stream (stitching is out of scope on a stream)")
        if args.track_smooth is not None or args.track_predict is not None:
            ap.error("--track-stitch does not go with --track-smooth or --track-predict (the smoother's completed table assumes "
                     "tracks seen within max_age frames)")
        try:
            from attend_infer_repeat_amd.stacks import stitch_spec
            parts = args.track_stitch.split(",") if args.track_stitch else []
            if len(parts) > 2:
                raise ValueError("at most two values")
            track_stitch = dict(max_gap=int(parts[0])) if parts else {}
            if len(parts) == 2:
                track_stitch["gate"] = float(parts[1])
            stitch_spec(track_stitch or True)
            track_stitch = track_stitch or True
        except ValueError as e:
            ap.error("--track-stitch needs MAX_GAP[,D2] with an integer MAX_GAP >= 1 and a squared distance D2 > 0, or no value, got %r (%s)"
                     % (args.track_stitch, e))
    if args.track_stream is not None:
        if track_eval is None:
            ap.error("--track-stream goes with --track-eval")
        if not 1 <= args.track_stream <= 32767 // 3:
            ap.error("--track-stream needs 1 <= CHUNK <= %d (CHUNK * max_steps must fit int16)" % (32767 // 3))
    stream_smooth = None
    if args.track_stream_smooth is not None:
        if args.track_stream is None:
            ap.error("--track-stream-smooth goes with --track-stream")
        try:
            lag_hz = [int(v) for v in args.track_stream_smooth.split(",")]
        except ValueError:
            lag_hz = []
        if len(lag_hz) not in (1, 2) or not 0 <= lag_hz[0] <= 16 or not 0 <= (lag_hz + [0])[1] <= 16:
            ap.error("--track-stream-smooth needs LAG[,HZ] with LAG and HZ within 0..16, got %r" % args.track_stream_smooth)
        stream_smooth = dict(lag=lag_hz[0], horizon=(lag_hz + [0])[1])
    if args.track_fit_noise is not None:
        if track_eval is None:
            ap.error("--track-fit-noise goes with --track-eval")
        if args.track_fit_noise < 0 or (args.track_fit_noise > 0 and args.eval_batches > 1):
            ap.error("--track-fit-noise needs ZOOM >= 0, and ZOOM > 0 needs --eval-batches 1 (the zoom re-runs on one batch's tracks)")
    track_motion = None
    if args.track_motion is not None:
        if track_eval is None:
            ap.error("--track-motion goes with --track-eval")
        track_motion = True
        if args.track_motion:
            try:
                qs, qc, r, vv = (float(v) for v in args.track_motion.split(","))
                from attend_infer_repeat_amd.track import check_motion
                track_motion = check_motion(dict(process_noise=(qs, qc), measurement_noise=r, velocity_var=vv))
            except ValueError as e:
                ap.error("--track-motion needs QS,QC,R,VV inside the smoother's noise domain or no value, got %r (%s)" % (args.track_motion, e))
    track_motion_gate = None
    if args.track_motion_gate is not None:
        if track_motion is None:
            ap.error("--track-motion-gate goes with --track-motion")
        try:
            from attend_infer_repeat_amd.track import check_motion_gate
            track_motion_gate = check_motion_gate(float(args.track_motion_gate) if args.track_motion_gate else True, track_motion)
        except ValueError as e:
            ap.error("--track-motion-gate needs a squared distance D2 > 0 or no value, got %r (%s)" % (args.track_motion_gate, e))
    track_smooth = None
    if args.track_smooth is not None or args.track_predict is not None:
        if track_eval is None:
            ap.error("--track-smooth and --track-predict go with --track-eval")
        track_smooth = {}
        if args.track_smooth:
            try:
                qs, qc, r = (float(v) for v in args.track_smooth.split(","))
            except ValueError:
                ap.error("--track-smooth needs QS,QC,R (three positive numbers) or no value, got %r" % args.track_smooth)
            if not (qs > 0 and qc > 0 and r > 0):
                ap.error("--track-smooth needs three positive numbers, got %r" % args.track_smooth)
            track_smooth.update(process_noise=(qs, qc), measurement_noise=r)
        if args.track_predict is not None:
            if not 1 <= args.track_predict <= 16:
                ap.error("--track-predict needs 1 <= HZ <= 16, got %r" % args.track_predict)
            track_smooth["horizon"] = args.track_predict
        track_smooth = track_smooth or True

    learning_rate, n_steps, batch_size = args.learning_rate, 3, 64    # multi_mnist.py:24-25,37
    num_steps_prior = AttrDict(anneal='exp', init=1. - 1e-15, final=1e-7, steps_div=1e4, steps=1e5, hold_init=1e3)
    appearance_prior = AttrDict(loc=0., scale=1.)
    where_scale_prior = AttrDict(loc=0., scale=1.)
    where_shift_prior = AttrDict(loc=0., scale=1.)
    step_bias, transform_var_bias, output_multiplier, init_explore_eps, l2_weight = .75, .5, .5, 1e-3, 0.

    device = torch.device("cuda", 0)
    torch.manual_seed(args.seed)                                      # parameter initialisation (Sonnet draws at build time)
    logdir = osp.join(args.results_dir, args.run_name)
    os.makedirs(logdir, exist_ok=True)
    tr, va = osp.join(args.data_dir, "mnist_train.pickle"), osp.join(args.data_dir, "mnist_validation.pickle")
    if osp.exists(tr) and osp.exists(va):
        train_data, valid_data = load_data(tr), load_data(va)
    elif args.glyphs:
        print("no multi-MNIST pickles under {!r}: procedural digit templates through the reference's generator".format(args.data_dir))
        as_float = lambda d: dict(imgs=d["imgs"].astype("float32") / 255.0, nums=d["nums"].astype("float32"))
        train_data = as_float(procedural_multi_mnist(args.synthetic_samples, seed=args.seed))
        valid_raw = procedural_multi_mnist(max(args.synthetic_samples // 6, batch_size), seed=args.seed + 1000,
                                           return_annotations=args.parse_score)
        valid_data = as_float(valid_raw)
        if args.parse_score:
            valid_data.update(boxes=valid_raw["boxes"], instances=valid_raw["instances"])
    else:
        print("no multi-MNIST pickles under {!r}: using a synthetic dataset".format(args.data_dir))
        train_data = synthetic_dataset(args.synthetic_samples, seed=args.seed)
        valid_data = synthetic_dataset(max(args.synthetic_samples // 6, batch_size), seed=args.seed + 1)
    if args.parse_score and not ("boxes" in valid_data and "instances" in valid_data):
        ap.error("--parse-score needs annotated validation data (boxes and instances): pass --glyphs, or write the pickles with "
                 "create_dataset.py --annotations; the stroke-blob synthetic dataset has no annotations")
    train_feed = DeviceFeeder(train_data, batch_size, device, shuffle=True, seed=args.seed)
    valid_feed = DeviceFeeder(valid_data, batch_size, device, shuffle=False)
    x, y = train_feed()

    n_hiddens = [32 * 8] * 2
    air = AIRonMNIST(x, y, max_steps=n_steps, explore_eps=init_explore_eps, inpt_encoder_hidden=n_hiddens,
                     glimpse_encoder_hidden=n_hiddens, glimpse_decoder_hidden=n_hiddens,
                     transform_estimator_hidden=n_hiddens, steps_pred_hidden=[128, 64], baseline_hidden=[256, 128],
                     transform_var_bias=transform_var_bias, step_bias=step_bias, output_multiplier=output_multiplier,
                     guard_degenerate=args.guard_degenerate or None)
    step_kw = {}
    if args.decay_rate is not None:
        step_kw["decay_rate"] = args.decay_rate
    if args.iw_train is not None:
        step_kw.update(use_engine=False, iw_samples=args.iw_train, iw_objective=args.iw_objective)
    train_step, global_step = air.train_step(learning_rate, l2_weight, appearance_prior, where_scale_prior,
                                             where_shift_prior, num_steps_prior, **step_kw)
    if args.init_from_tf_ckpt:
        from attend_infer_repeat_amd.tf_checkpoint import global_step_of, import_tf_checkpoint, import_tf_optimizer_slots, mapping_report
        name_map = None
        if args.tf_name_map:
            name_map = json.load(open(args.tf_name_map))
        named = import_tf_checkpoint(args.init_from_tf_ckpt, air._engine.param_shapes, name_map=name_map)
        air._engine.load_parameters({k: torch.from_numpy(v) for k, v in named.items()})
        air._engine.reset_optimizer()
        slots = import_tf_optimizer_slots(args.init_from_tf_ckpt, air._engine.param_shapes, name_map=name_map)
        left = mapping_report(args.init_from_tf_ckpt, air._engine.param_shapes, name_map)
        if left["unmapped_engine_parameters"]:
            print('WARNING: not in the checkpoint (kept at their initial values): {}'.format(', '.join(left["unmapped_engine_parameters"])))
        if left["unused_checkpoint_variables"]:
            print('WARNING: checkpoint variables nobody used (pass --tf-name-map if one of them belongs to the model): {}'.format(
                ', '.join(left["unused_checkpoint_variables"])))
        half = [n for n in named if n not in slots['ms']]
        if half and slots['ms']:
            print('WARNING: no complete RMSProp slots in the checkpoint for: {}'.format(', '.join(sorted(half))))
        air._engine.load_optimizer_slots(**{k: {n: torch.from_numpy(v) for n, v in d.items()} for k, d in slots.items()})
        step0 = global_step_of(args.init_from_tf_ckpt)
        if step0 is not None:
            air._engine.set_global_step(step0); air.global_step.fill_(step0)
        print('Initialised {} tensors (+ RMSProp slots of {}) from {} (global_step {})'.format(len(named), len(slots['ms']), args.init_from_tf_ckpt, step0))
        global_step = air.global_step
    if args.resume:
        # the reference only ever saves (tf.train.Saver over every variable incl. the optimiser slots and global_step,
        # multi_mnist.py:116,145-146); restoring is the counterpart a long run needs
        ck = torch.load(args.resume, map_location="cpu")
        air._engine.load_state_dict(ck["engine"])
        air.global_step.fill_(int(ck["engine"]["global_step"]))
        if "train_feed" in ck:
            train_feed.load_state_dict(ck["train_feed"]); valid_feed.load_state_dict(ck["valid_feed"])
        global_step = air.global_step
    if args.device_feeder:
        air._engine.attach_dataset(train_feed.imgs.reshape(train_feed.n, -1), shuffle=True, seed=args.seed)
        air._engine.capture()
    writer = open(osp.join(logdir, "log.jsonl"), "a")
    log = make_logger(air, train_feed, args.eval_batches, valid_feed, args.eval_batches, writer)
    if args.iw_particles > 0:
        plain_log = log
        iw_log = make_iw_logger(air, valid_feed, args.eval_batches, args.iw_particles, 'test', writer)

        def log(train_itr):                               # noqa: F811
            out = plain_log(train_itr)
            iw_log(train_itr)
            return out

    if args.prior_samples > 0:
        inner_log = log

        def log(train_itr):                               # noqa: F811
            out = inner_log(train_itr)
            counts = air.sample_scenes(args.prior_samples).generated_num_objects
            hist = torch.bincount(counts.to(torch.int64), minlength=n_steps + 1).tolist()
            print('Step {}, prior samples: counts 0..{} = {}'.format(train_itr, n_steps, hist))
            writer.write(json.dumps(dict(step=int(train_itr), data="prior_samples", n_scenes=int(args.prior_samples),
                                         count_probs="model", count_hist=hist)) + "\n"); writer.flush()
            if args.figures:
                make_prior_fig(air, logdir, train_itr)
            return out

    parse_kw = dict(particles=args.parse_particles, select=args.parse_select) if args.parse_particles > 0 else {}
    if args.parse_eval:
        before_parse_log = log
        parse_log = make_parse_logger(air, valid_feed, args.eval_batches, 'test', writer, **parse_kw, **refine_kw)

        def log(train_itr):                               # noqa: F811
            out = before_parse_log(train_itr)
            parse_log(train_itr)
            if args.figures:
                make_parse_fig(air, logdir, train_itr, **parse_kw)
            return out

    if args.parse_score:
        before_score_log = log
        score_log = make_parse_score_logger(air, valid_data, args.eval_batches, 'test', writer, **parse_kw, **refine_kw)

        def log(train_itr):                               # noqa: F811
            out = before_score_log(train_itr)
            score_log(train_itr)
            return out

    if tiled is not None:
        from attend_infer_repeat_amd.evaluation import make_tiled_parse_score_logger
        scenes_per_batch = 16
        raw = procedural_multi_mnist(scenes_per_batch * max(args.eval_batches, 1), canvas_size=tiled["scene"],
                                     n_objects=(0, args.parse_tiled_objects), seed=args.seed + 1000, n_templates=256,
                                     return_annotations=True)            # the validation set's generator and its first templates
        scene_data = dict(imgs=raw["imgs"].astype("float32") / 255.0, boxes=raw["boxes"], instances=raw["instances"])
        before_tiled_log = log
        tiled_log = make_tiled_parse_score_logger(air, scene_data, args.eval_batches, 'test', scenes_per_batch, writer,
                                                  stride=tiled["stride"], **refine_kw)

        def log(train_itr):                               # noqa: F811
            out = before_tiled_log(train_itr)
            tiled_log(train_itr)
            return out

    if track_eval is not None:
        from attend_infer_repeat_amd.data import procedural_moving_mnist
        from attend_infer_repeat_amd.evaluation import make_track_score_logger
        sequences_per_batch = 16
        raw = procedural_moving_mnist(sequences_per_batch * max(args.eval_batches, 1), track_eval["frames"],
                                      canvas_size=tuple(int(v) for v in air.obs.shape[-2:]),
                                      n_objects=(0, 2), speed=(min(1.0, track_eval["speed"]), track_eval["speed"]), spans=True,
                                      seed=args.seed + 2000, n_templates=256, return_annotations=True)
        seq_data = dict(imgs=raw["imgs"].astype("float32") / 255.0, boxes=raw["boxes"], instances=raw["instances"])
        before_track_log = log
        track_log = make_track_score_logger(air, seq_data, args.eval_batches, 'test', sequences_per_batch, writer, temporal=track_temporal,
                                            smooth=track_smooth, matching=args.track_matching, identity=args.track_identity,
                                            motion=track_motion, motion_gate=track_motion_gate, hota=args.track_hota, stitch=track_stitch,
                                            mots=args.track_mots, **refine_kw)

        stream_log = None
        if args.track_stream is not None:
            from attend_infer_repeat_amd.evaluation import make_track_stream_logger
            stream_log = make_track_stream_logger(air, seq_data, args.eval_batches, 'test', args.track_stream, sequences_per_batch, writer,
                                                  temporal=track_temporal, matching=args.track_matching, **refine_kw)
            if stream_smooth is not None:
                plain_log, smooth_log = stream_log, make_track_stream_logger(
                    air, seq_data, args.eval_batches, 'test', args.track_stream, sequences_per_batch, writer, smooth=stream_smooth,
                    temporal=track_temporal, matching=args.track_matching, **refine_kw)
                stream_log = lambda *a, **kw: (plain_log(*a, **kw), smooth_log(*a, **kw))[0]

        fit_log = None
        if args.track_fit_noise is not None:
            from attend_infer_repeat_amd import trajectory as tj
            D = tj.DEFAULTS
            at_defaults = tuple(q / D["measurement_noise"] for q in D["process_noise"])
            grid = tuple(sorted(set(tj.DEFAULT_FIT_RATIOS + at_defaults)))      # the defaults' own ratios are candidates too

            def fit_log(train_itr):
                n = min(max(args.eval_batches, 1), seq_data["imgs"].shape[0] // sequences_per_batch)
                kw = dict(temporal=track_temporal, matching=args.track_matching, **refine_kw)
                if track_motion is not None:
                    kw["motion"] = track_motion                    # the tracks the terms are fitted to are the ones being evaluated
                if track_motion_gate is not None:
                    kw["motion_gate"] = track_motion_gate
                rec = dict(step=train_itr, data="test_track_noise_fit", zoom=args.track_fit_noise)
                try:
                    for b in range(n):
                        sl = slice(b * sequences_per_batch, (b + 1) * sequences_per_batch)
                        fit = air.fit_track_noise(torch.as_tensor(seq_data["imgs"][sl], dtype=torch.float32).to(air.obs.device), grid, grid,
                                                  zoom=args.track_fit_noise, accumulate=b > 0, fit=b == n - 1, **kw)
                    fitter = air.noise_fitter(sequences_per_batch, track_eval["frames"], grid, grid, **kw)
                    first = fitter.read_totals()                   # the first grid's totals: the defaults' ratios are cells of it
                    i, j = grid.index(at_defaults[0]), grid.index(at_defaults[1])
                    rec.update(process_noise=list(fit["process_noise"]), measurement_noise=fit["measurement_noise"],
                               velocity_var=fit["velocity_var"], n_innovations=fit["n_innovations"], cell=list(fit["cell"]),
                               on_edge=list(fit["on_edge"]), loglik_per_innovation=fit["loglik"] / fit["n_innovations"],
                               loglik_per_innovation_at_defaults=tj.profile_loglik(first, i, j, D["measurement_noise"]) / fit["n_innovations"])
                    if any(fit["on_edge"]):
                        print("warning: the fitted noise terms lie on the edge of the grid %s: the maximum may be outside it"
                              % (fit["on_edge"],))
                except ValueError as e:                            # no track with two sightings, every innovation zero, ...
                    rec["refused"] = str(e)
                print("{}: test_track_noise_fit {}".format(train_itr, {k: v for k, v in rec.items() if k not in ("step", "data")}))
                writer.write(json.dumps(rec) + "\n"); writer.flush()
                if track_motion is not None and "refused" not in rec:      # the identity figures with motion at the defaults and at the fit
                    fitted = {k: fit[k] for k in tj.FIT_KEYS}
                    for tag, terms in (("defaults", True), ("fit", fitted)):
                        make_track_score_logger(air, seq_data, args.eval_batches, 'test_motion_' + tag, sequences_per_batch, writer,
                                                temporal=track_temporal, matching=args.track_matching, identity=args.track_identity,
                                                motion=terms, motion_gate=track_motion_gate, **refine_kw)(train_itr)

        def log(train_itr):                               # noqa: F811
            out = before_track_log(train_itr)
            track_log(train_itr)
            if stream_log is not None:
                stream_log(train_itr)
            if fit_log is not None:
                fit_log(train_itr)
            return out

    train_itr = int(global_step)
    print('Starting training at iter = {}'.format(train_itr))
    if train_itr == 0:
        log(0)
    t0, last = time.time(), train_itr
    iw_degenerate_total = 0
    while train_itr < args.iters:
        if args.device_feeder:
            train_itr = int(train_step(None, None, refresh=False))
        elif args.iw_train is not None:
            xb, yb = train_feed()
            train_itr = int(train_step(xb, yb))
            iw_degenerate_total = iw_degenerate_total + air.iw_degenerate      # (a device tensor: no sync per step)
        else:
            xb, yb = train_feed()
            train_itr = int(train_step(xb, yb, refresh=False))
        if args.check_every and train_itr >= args.check_from and train_itr % args.check_every == 0:
            eng = air._engine
            o = eng.outputs()
            fin = lambda t: bool(torch.isfinite(t).all().item())
            diag = dict(step=train_itr, data="check",
                        where_scale_min=float(o["where_scale"].min()), where_scale_max=float(o["where_scale"].max()),
                        what_scale_min=float(o["what_scale"].min()), what_scale_max=float(o["what_scale"].max()),
                        where_abs_max=float(o["where"].abs().max()), what_abs_max=float(o["what"].abs().max()),
                        presence_prob_min=float(o["presence_prob"].min()), presence_prob_max=float(o["presence_prob"].max()),
                        num_step=float(o["num_step_per_sample"].mean()), rec=float(o["rec_loss"]),
                        kl_what=float(o["kl_what"]), kl_where=float(o["kl_where"]),
                        imp_var=float(o["imp_weight_var"]), baseline_abs_max=float(o["baseline"].abs().max()),
                        params_abs_max=float(eng.flat_params.abs().max()), grads_abs_max=float(eng.flat_grads.abs().max()),
                        ms_max=float(eng.flat_ms.max()), ms_min=float(eng.flat_ms.min()), mom_abs_max=float(eng.flat_mom.abs().max()),
                        finite=dict(params=fin(eng.flat_params), grads=fin(eng.flat_grads), ms=fin(eng.flat_ms), mom=fin(eng.flat_mom)))
            # the variance slot of centred RMSProp, ms - mg^2, must stay >= 0 for the square root (model.py:265: centered=True)
            diag["centred_var_min"] = float((eng.flat_ms - eng.flat_mg * eng.flat_mg).min())
            worst = {}
            for k, g in eng.named_grads().items():
                worst[k] = float(g.abs().max())
            top = sorted(worst.items(), key=lambda kv: -kv[1] if kv[1] == kv[1] else -float("inf"))[:3]
            diag["largest_grads"] = top
            writer.write(json.dumps(diag) + "\n"); writer.flush()
        if args.iw_train is not None:
            if args.summary_every and train_itr % args.summary_every == 0:
                writer.write(json.dumps(dict(step=train_itr, data="summary", iw_samples=args.iw_train, iw_objective=air.iw_objective,
                                             iw_bound=float(air.iw_bound),
                                             iw_ess=float(air.iw_ess), iw_degenerate=int(air.iw_degenerate),
                                             iw_degenerate_total=int(iw_degenerate_total), rec=float(air.rec_loss),
                                             loss=float(air.loss.value), opt_loss=float(air.opt_loss), num_step=float(air.num_step),
                                             num_step_acc=float(air.num_step_accuracy))) + "\n")
        elif args.summary_every and train_itr % args.summary_every == 0:
            # the reference's `all_summaries` (model.py's tf.summary scalars + evaluation.gradient_summaries), every 1000 iterations
            writer.write(json.dumps(dict(step=train_itr, data="summary", **step_summaries(air, histogram=args.grad_histograms))) + "\n")
        if train_itr % args.log_every == 0:
            torch.cuda.synchronize()
            dt = time.time() - t0
            print("iter {}: {:.0f} images/s".format(train_itr, (train_itr - last) * batch_size / max(dt, 1e-9)))
            log(train_itr)
            t0, last = time.time(), train_itr
        if train_itr % args.save_every == 0 and args.iw_train is not None:
            torch.save({"cell": air.cell.state_dict(), "global_step": train_itr, "iw_samples": args.iw_train,
                        "iw_objective": air.iw_objective},
                       osp.join(logdir, "model_{}.pt".format(train_itr)))
        elif train_itr % args.save_every == 0:
            torch.save({"engine": air._engine.state_dict(), "train_feed": train_feed.state_dict(),
                        "valid_feed": valid_feed.state_dict()}, osp.join(logdir, "model_{}.pt".format(train_itr)))
            if args.figures:
                make_fig(air, logdir, train_itr)
    writer.close()
    return air


if __name__ == "__main__":
    main()
