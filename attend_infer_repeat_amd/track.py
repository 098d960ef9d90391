"""Tracking objects across the frames of a sequence on the device: the per-frame parses of a bound provider in, identities out.

A sequence of F frames is F rows of a parser, and its parse is F unrelated object lists: slot t of frame f has nothing to do with slot
t of frame f + 1.  This module associates them -- tracking by association: no latent is carried from one frame into the next frame's
inference, the assignment is greedy by default (the house rule of air_score_match and air_tile_merge) or, with matching="optimal", the
exact optimum of the frame (Hungarian), and the metrics are CLEAR-MOT and, on request, IDF1.

Layout.  The provider has R = S F rows, sequence-major: row r = s F + f (the tile layout r = s Nw + v, with frames for windows).
1 <= T <= 32 objects per frame, F T <= 32767 (a track id fits the int16 of `track_owner`).

The association rule (air_track_associate; include/air_hip.h states the same).  Each sequence on its own, the frames in ascending order,
a table of at most 32 LIVE tracks: slot, id, the (frame, slot) of the last sighting, age (frames since that sighting), length, gaps.
For frame f with n = clip(num_objects[r], 0, T), in this order:
  1. states: object j >= n is ABSENT; j < n is NONFINITE if any of its four box values, its score or its A `what` values is not finite,
     and takes no further part.
  2. affinity of every live track k and finite object j:  iou = air_score_match's float64 box IoU of the track's last-sighting box and
     the object's box;  msd = (sum_a (what_k[a] - what_j[a])^2) / A in float64 from the widened fp32 values, summed in ascending a;
     aff = (1 - w) * iou + w / (1 + msd).  Admissible iff iou > iou_gate, strictly.  No transcendental function: device and numpy agree
     to the bit.
  3. greedy matching: while an admissible pair of an unmatched track and an unmatched object exists, the one with the largest aff (equal
     aff: the lower track id, then the lower j): the object is MATCHED with the track's id, prev_frame / prev_slot = the track's last
     sighting, affinity = aff rounded once to fp32;  the track: gaps += (age > 0), age = 0, length += 1, last sighting (f, j).
  4. births: the unmatched finite objects in ascending j:  score >= birth_score: BORN with id = next_id++ in the lowest free slot, or
     OVERFLOW (id -1) when no slot is free;  score < birth_score: UNCONFIRMED (id -1).  Matching ignores birth_score, so an object
     below it still continues an existing track.
  5. ageing: every live track neither matched nor born in this frame gets age += 1; one with age > max_age is retired, its slot is
     free from frame f + 1 on.  Ids are never reused.
So a track survives max_age frames without a sighting: with max_age = 1 an object missing in one frame comes back under its id, and a
slot held by a track last seen in frame f is free again in frame f + max_age + 2.

Optimal matching (matching="optimal": air_track_associate_optimal).  Steps 1, 2, 4 and 5 as above; step 3 becomes:
  3. rows: the finite objects, ascending j.  Columns: the 32 track slots, and for each object one "stays unmatched" column of its own.
     profit(k, j) = 1 + floor(aff * 2^32) as int64 for an admissible pair (the product by a power of two is exact; the 1 makes any
     admissible pair beat staying unmatched), 0 for staying unmatched; an inadmissible pair is forbidden.  The matches are the
     one-to-one assignment of the largest summed profit; all solver arithmetic is int64, so that sum is exact and the same for every
     correct solver.  Among several assignments of that sum: the one `solve_assignment` yields -- a shortest-augmenting-path Hungarian
     that inserts the objects in ascending j, grows the alternating tree from the inserted object by the unused column of the least
     reduced cost (equal: the lowest column, slots before the unmatched columns; a column keeps the first tree column that gave it
     that cost as its predecessor) until a free column is reached, and moves the rows along that path.  Every matched pair is booked
     as in the greedy step 3.  Matching still ignores birth_score, and a NaN still never matches.
The greedy rule takes the best pair first and can leave a second object without an admissible partner -- a spurious birth, a coasting
track and an identity switch where two objects are close or cross; the optimal rule looks at the whole frame.

MOTION (motion=True | dict: air_track_associate_motion, either matching; `reference_associate_motion` restates it).  The rule above has no
notion of motion: a track that coasts over a frame or two while its object moves finds the object where its old box no longer reaches
-- a new id, a fragmented track --, and in the frame after two objects cross each track's last box lies on the OTHER object.  With
motion every live track is matched against where it is predicted to be.  Steps 1-5 (3' for "optimal") stay, with these exceptions:
  state    each live track carries the FILTERED state of the trajectory filter (trajectory.py: start / predict / update) at its last
           sighting, in float64: x[4] and v[4] over [sx, tx, sy, ty] and (Pxx, Pxv, Pvv) per noise class -- shifts tx, ty with q_shift,
           scales sx, sy with q_scale --, 14 doubles per track.
  step 1   an object whose `where` row holds a non-finite value is NONFINITE as well.
  step 2   for live track k last sighted at frame l, m = f - l >= 1:  pred_where = float32([x_sx, x_tx + m v_tx, x_sy, x_ty + m v_ty]),
           exactly trajectory._forecast_where(x, v, m): shifts extrapolated, scales held, one product and one sum in float64, rounded
           once;  pred_box = tile.scene_boxes(pred_where, img_size) in fp32, operation by operation;  if any of its four values is not
           finite, pred_box is the last-sighting box;  iou = the unchanged float64 box IoU of pred_box and the object's box.  The gate,
           msd, aff, the profit and every tie order are unchanged.
  booking a match (k, j): as in step 3, and the state advances by trajectory._filter_step, verbatim: m - 1 times without a sighting
           (predict only, one frame at a time, never as m v), then once with z = the object's `where` row widened to float64.
  a birth  starts the state: trajectory._filter_start(z, measurement_noise, velocity_var).
Two more outputs, pred_where and pred_boxes [T, R, 4] fp32: for a MATCHED object the prediction of its track that the match was made
against, zero in every other row.  process_noise=(q_shift, q_scale), measurement_noise and velocity_var are what `smooth=` and
`fit_track_noise` use, and must lie in the smoother's supported domain (trajectory.check_arguments raises, the entry returns
AIR_E_SHAPE).  EXACT CONSEQUENCES:
  1. zero velocity.  While a track's v is exactly 0 its prediction is its last `where` row bit for bit -- every track at its first
     association after its birth, and a track whose sightings all carry one value.  Hence on sequences whose tracks are all static,
     with boxes == scene_boxes(where), every output equals air_track_associate's / _optimal's bit for bit; and so on ANY input with
     F <= 2.
  2. one filter.  For a MATCHED object of track i in frame f, pred_where equals the fc_where row of track i, column k = 1, of
     trajectory.reference_smooth(..., horizon=1) run on this tracker's own output restricted to the frames 0 .. f - 1 (track_last
     recomputed from track_id, num_tracks = the ids issued before f): the filter inside the tracker and the smoother behind it are
     one filter, and the state at a track's last sighting is the forward pass of `reference_smooth` on that track, bit for bit.
A track has v = 0 until its second sighting: an object displaced by more than its box in its first step is linked by neither rule
-- THE GATE below links it.
THE GATE (motion_gate=True | G with motion=: air_track_associate_motion_gated, either matching; `reference_associate_motion(gate=)`
restates it; motion_gate=None is exactly MOTION above).  MOTION uses the filter's predicted MEAN alone: the covariance it carries says
how far a sighting may plausibly lie from that mean -- far for a newborn track, whose rate is unknown (velocity_var), near for a track
followed for many frames -- and the IoU gate knows neither.  G is a squared Mahalanobis distance, finite and > 0; True is
MOTION_GATE_DEFAULT = 13.2767, the 0.99 quantile of chi-squared with 4 degrees of freedom (provisional like the other association
defaults: unmeasured on a trained model).  Steps 1-5 of MOTION stay; step 2 changes:
  per track  for live track k last sighted at l, m = f - l >= 1: the PREDICTED state of its filter m frames on, by the statements a
           match would run -- the m - 1 coasted frames predicted one by one (x = x + v and the covariance predict), then one more
           predict: xp[4] and Pxx- per noise class; never m v.  s[cl] = Pxx-[cl] + measurement_noise.
  per pair   (k, j) with a finite object j, in float64: e[c] = z[c] - xp[c] over [sx, tx, sy, ty], z = the object's `where` row
           widened;  d2 = ((e0 e0 / s_scale + e1 e1 / s_shift) + e2 e2 / s_scale) + e3 e3 / s_shift.  Admissible iff d2 <= G (a NaN or an
           inf fails); iou_gate is NOT applied.  aff = (1 - w) / (1 + d2) + w / (1 + msd): rational, within [0, 1], no transcendental.
           The int64 profit, the greedy and the optimal step 3 and every tie order are unchanged.
pred_where and pred_boxes stay the forecast row (scales held) and its box.  One more output, pred_d2 [T, R] fp32: for a MATCHED object
float32(d2) of the pair that was matched, zero in every other row.  Booking a match, the advance of the state, births and ageing are
MOTION's.  EXACT CONSEQUENCES:
  1. for a MATCHED object pred_d2 is float32(sum e^2 / s) with (xp, Pxx-) the predicted tuple of trajectory._filter_step applied to the
     track's filtered state, the coasted frames first, e = z - xp and s = Pxx- + r: the innovation and its variance of the very update
     that books the match -- the quantities whose likelihood `fit_track_noise` maximises.
  2. consequence 2 of MOTION holds under the gate: the final states equal the smoother's forward pass on the tracker's own output.
`return_margins=True` reports gate_margin = min |d2 - G| under the gate.
Out of scope: motion or the gate on a stream (StreamTracker refuses both: the carried state would need the 14 doubles per slot, and
its chunk-invariance tests), a gate per component, rates on scales in pred_where, feeding smoothed (non-causal) rows back, motion for
the temporal proposer.  What motion, the gate and the gate's default threshold do to MOTA / IDF1 on the parses of a TRAINED model is
unmeasured (profiles/track_motion.txt and profiles/track_gate.txt say what was measured: the cost of the tail).

The identity metric (air_track_score).  gt_boxes [R, G, 4], G <= 8: ground-truth slot g is the SAME object in every frame of a sequence,
width <= 0 = absent in that frame.  The hypotheses of a frame are its objects j < n with track_id >= 0 and finite boxes.  map[g] = none
at the start of a sequence.  Per frame:
  1. for g ascending: a present g whose map[g] is the id of a hypothesis j not yet taken with iou(gt_g, box_j) > tau keeps j;
  2. the remaining present g and hypotheses greedily by float64 IoU descending, strictly > tau (equal: the lower g, then the lower j);
  3. for every matched (g, j) in ascending g: idsw += (map[g] exists and != id_j), then map[g] = id_j (map persists while g is unmatched
     or absent);
  4. gt += present g, matches, misses += present unmatched g, fp += unmatched hypotheses, sum_iou += the matches' iou (float64, frame
     order, then g order), tracked[g] / present[g] += 1.
seq_counts [S, 8] = {gt, matches, misses, fp, idsw, mostly tracked (5 tracked[g] >= 4 present[g]), mostly lost (5 tracked[g] <=
present[g]), gt objects}, the last three over g with present[g] > 0, in integers.

IDF1 (air_track_idf; Ristani et al. 2016: how long each ground-truth object keeps ONE identity, where MOTA counts a switch once and
forgets it).  Hypotheses and present ground-truth slots as above.  overlap[s, g, id] = the number of (frame, hypothesis) pairs in which
present g and a hypothesis with that id have float64 IoU > tau, strictly (an id twice in a frame counts once per hypothesis; an id >=
n_ids is ignored).  idtp = the largest sum of overlap[s, g, id] over one-to-one assignments of slots to ids: exact, by dynamic
programming over the 2^G subsets of slots, the ids visited in ascending order.  seq_idf [S, 4] = {idtp, gt_frames (present g summed over
the frames), hyp_frames (hypotheses summed over the frames), ids with overlap}.  On the host: IDFN = gt_frames - idtp, IDFP = hyp_frames
- idtp, IDP = idtp / hyp_frames, IDR = idtp / gt_frames, IDF1 = 2 idtp / (gt_frames + hyp_frames); a denominator of 0 gives nan.

HOTA (air_track_hota; Luiten et al., IJCV 2021, the figure TrackEval reports: HOTA = sqrt(DetA AssA) averaged over 19 localisation
thresholds -- DetA says how well objects are found, AssA how well the matched detections are kept together in one identity, LocA how
well the matches are localised; MOTA is dominated by detection, IDF1 is one global match at one tau).  Inputs as for air_track_idf.
Hypotheses of a frame and present slots as above; a hypothesis whose id is >= n_ids takes no part in any table or matching (its sim
is 0 everywhere, it is no row of the matching, it adds to no count but hyp_dets) and so counts as an unmatched hypothesis.  sim[g, j]
= the float64 box IoU of a present slot g and a hypothesis j (id < n_ids), 0 otherwise.  Everything a float decides is float64 with
contraction off, only + - * / and floor, in the order written here; no transcendental and no square root on the device.  Thresholds:
alpha_k = k / 20.0, k = 1..19 (HOTA_ALPHAS), computed that way on the device too; a match counts at alpha_k iff sim >= alpha_k.
  pass 1, the frames in order:  rs[g] = sum_j sim[g, j] in ascending j, cs[j] = sum_g sim[g, j] in ascending g;  for every present g and
          hypothesis j, in ascending j:  d = (cs[j] + rs[g]) - sim[g, j], and if d > 2^-52:  pot[g, id_j] += sim[g, j] / d  (an id
          twice in a frame adds twice; a pair with sim = 0 adds +0: no change of bits);  gc[g] += 1 per present slot, ic[id_j] += 1 per
          hypothesis.
  pass 2, the frames in order:  (g, j) is admissible iff sim[g, j] > 0;  A = pot[g, id] / ((gc[g] + ic[id]) - pot[g, id]) with the
          counts widened to float64;  profit = 1 + (int64) floor((A sim) 2^32).  ONE matching per frame, whatever the threshold: the
          exact optimal assignment of `solve_assignment` (air_track_associate_optimal's solver and tie rule, above) with the
          hypotheses in ascending j as rows, the slots g < G as columns and every other slot column forbidden.  For every matched
          (g, j) in ascending g, with L = the number of k with sim >= alpha_k:  for a < L:  tp[a] += 1, loc[a] += sim,
          matches[a, g, id_j] += 1.  gt_dets += present slots, hyp_dets += hypotheses (those with an id >= n_ids included).
  the end of the sequence:  fn[a] = gt_dets - tp[a], fp[a] = hyp_dets - tp[a];  with c = matches[a, g, id] over c > 0, the counts
          widened:  ass[a] = sum c (c / ((gc[g] + ic[id]) - c)), ass_re[a] = sum c (c / gc[g]), ass_pr[a] = sum c (c / ic[id]) -- per
          (a, g) over the ids in ascending order, then per a over g in ascending order.
Outputs per sequence, every element written: seq_hota_i [S, 19, 3] int32 (HOTA_COUNTS: tp, fn, fp), seq_hota_f [S, 19, 4] float64
(HOTA_SUMS: ass, ass_re, ass_pr, loc), hota_potential [S, G, n_ids] float64, hota_id_count [S, n_ids], hota_gt_count [S, G],
hota_matches [S, 19, G, n_ids] int32.  `hota_summary` combines sequences in TrackEval's way: the counts and the numerators are summed,
then per threshold DetA = tp / max(1, tp + fn + fp), DetRe = tp / max(1, tp + fn), DetPr = tp / max(1, tp + fp), AssA = ass / max(1,
tp) (AssRe, AssPr alike), LocA = loc / tp or 1 when tp = 0, HOTA_a = sqrt(DetA AssA) -- the only square root, on the host -- and the
figures are the means over the 19 thresholds; nan for every figure when there was neither ground truth nor a hypothesis.  TWO STATED
DEPARTURES from TrackEval: 1. the matching score A sim is quantised to 2^-32 (and 1 is added) for an exact integer solver with a stated
tie rule, where TrackEval hands floats to scipy's solver: the two can differ only where two assignments lie within 2^-32 per pair of
each other;  2. no epsilon at the thresholds: TrackEval counts sim >= alpha - eps, this rule sim >= alpha.  Out of scope: HOTA on a
stream (the tables are indexed by global id, as for IDF1), a mask similarity inside HOTA (MOTS, below, is where masks are scored),
thresholds other than the 19, HOTA per class.  The HOTA of a trained model's tracks is unmeasured (profiles/track_hota.txt says what
was measured: the cost of the launch).

MOTS (air_track_mots; Voigtlaender et al., CVPR 2019: MOTSA, sMOTSA, MOTSP -- the tracks scored as MASKS).  Objects overlap, the
renderer decides who owns a pixel, and the owner map records that decision; a box metric cannot see whether it was right.  Inputs:
cont [R, T+1, G+1] int32 exactly as air_score_contingency writes it for (the step owner map, the ground-truth instance map) --
cont[r, a, b] = the pixels with owner + 1 == a and gt + 1 == b; `mots_contingency` restates it --, num_objects [R] and the table's id
column track_id [T, R] (the tracker's, the stitcher's stitch_id, the smoother's completed ids).  Boxes are not read.  Per frame, every
sum in int64:  row[j] = sum_b cont[r, j+1, b], the hypothesis area;  col[g] = sum_a cont[r, a, g+1], the ground-truth area, the pixels
owned by the background and by steps that are no hypothesis included.  Hypotheses: the steps j < clip(num_objects[r], 0, T) with
track_id[j, r] >= 0 and row[j] > 0 -- a step without a track, or without a single pixel of its own, is neither a match nor a false
positive.  Slot g is present iff col[g] > 0.  For a present g and a hypothesis j:  inter = cont[r, j+1, g+1], union = row[j] + col[g] -
inter;  they match iff inter > union - inter: mask IoU > 1/2 with no float and no 2 inter that could overflow.  Within a frame the
hypothesis masks are disjoint and the ground-truth masks are disjoint, so for a non-negative table at most one j qualifies per g and
at most one g per j (a match holds more than half of both areas): the search order cannot change the result -- no Hungarian solver,
no tie rule, no threshold sweep, and NO tau argument, because uniqueness rests on the 1/2.  (Stated for completeness: the lowest
qualifying j of a slot is taken, and a hypothesis is unmatched iff no slot took it.)  For every matched (g, j) in ascending g:  tp +=
1;  soft += float64(inter) / float64(union), summed in frame order, then g order;  ids += (map[g] exists and != id_j), then map[g] =
id_j;  tracked[g] += 1.  map[g] is none at the start of a sequence and persists while g is unmatched or absent (step 3 of the
identity metric above; the paper's latest tracked predecessor).  gt += present g, fn += present unmatched g, fp += unmatched
hypotheses, present[g] += 1 per present g.  Outputs, every element written by one writer: seq_mots_i [S, 8] int32 (MOTS_COUNTS: gt,
tp, fn, fp, ids, mostly tracked (5 tracked[g] >= 4 present[g]), mostly lost (5 tracked[g] <= present[g]), gt objects -- the last
three over g with present[g] > 0), seq_mots_f [S] float64 = soft, mots_match [R, G] int32 (the matched step, -1 otherwise), mots_iou
[R, G] fp32 (the quotient rounded once, 0 otherwise).  `mots_summary`, on the host after one read-back: MOTSA = (tp - fp - ids) / gt,
sMOTSA = (soft - fp - ids) / gt, MOTSP = soft / tp, recall = tp / gt, precision = tp / (tp + fp), the mostly tracked / lost fractions;
a denominator of 0 gives nan.  Out of scope: MOTS on a stream (StreamTracker's carried score state has a fixed layout), ignore
regions, thresholds other than 1/2, a mask similarity inside HOTA or IDF1, sharing the contingency with a ParseScorer bound to the
same provider.  What sMOTSA a TRAINED model's tracks reach is unmeasured (profiles/track_mots.txt says what was measured: the cost
of the two launches).

STITCHING (air_track_stitch; `reference_stitch` restates it; `TrackStitcher` runs it behind a SequenceTracker).  A track that coasts more
than max_age frames is retired, and its object, when it comes back, is born again under a new id -- the split track that HOTA books
as AssA 0.5 and IDF1 as a lost half.  Raising max_age does not repair it (32 live slots, a completed table that grows with max_age, a
long-coasting track that takes the sightings of newborn ones).  Stitching is a second pass over WHOLE tracks, tracklet linking: a
track that ended is joined to one that began later when the motion filter of the first predicts where the second begins and their
`what` codes agree, the links chosen by ONE optimal assignment.  Inputs: the tracker's output (track_id, num_tracks, track_first,
track_last, track_length, track_gaps) and the provider rows it read (what [T, R, A], where [T, R, 4]); max_gap (an integer >= 1,
default 8), gate (a squared Mahalanobis distance, finite and > 0; True: MOTION_GATE_DEFAULT), appearance_weight w in [0, 1] and the
four noise terms of the trajectory filter (None: trajectory.DEFAULTS; `check_motion` holds them to the smoother's supported domain).
Each sequence s on its own, N = max(num_tracks[s], 0); N > 32 is OVERFLOW, below.
  filter   for every id i < N the forward filter of the trajectory smoother over the sightings of track i in frame order, the frames
           clip(track_first[i]) .. clip(track_last[i]) (clipped to 0 .. F - 1) walked one by one; track i is sighted in frame f at the
           lowest slot j with track_id[j, s F + f] == i.  The first sighting starts the filter as a birth does (x = z, v = 0, P = (r,
           0, velocity_var)); then `_motion_advance`'s statements: every frame without a sighting is predicted on its own, a sighting
           is a predict and an update.  The state at the last sighting is trajectory._filter_step's forward pass bit for bit -- the
           motion_state of `reference_associate_motion(return_state=True)` when the tracker ran with motion= and the same terms.  The
           frames of a track's first and last sighting are those this walk found (on the tracker's own output: track_first and
           track_last); an id without a sighting there takes no part.
  pair     (a, b), both with sightings: g = first[b] - last[a]; a candidate iff 1 <= g <= max_gap -- hence a != b, and a chain runs
           forward in time.  (xp, s) = `_motion_predicted_state(filt_a, g, q, r)`: the gate's statements with m := g, g predicts one
           by one, never g v.  z = the `where` row of b's FIRST sighting widened to float64; d2 = `_motion_d2(xp, s, z)` in the order
           [sx, tx, sy, ty]; msd = the association's mean squared difference (float64, ascending index, over A) of the `what` row of
           a's LAST sighting and that of b's first.  Admissible iff d2 <= gate (a NaN or an inf fails), and then aff = (1 - w) / (1 +
           d2) + w / (1 + msd) must be >= 0 (a NaN msd fails); profit = 1 + floor(aff 2^32).
  links    the exact optimal assignment of `solve_assignment`, the association's solver and tie rule: rows the ids b < N ascending,
           column a = track a, column 32 + b = "b keeps its id".  parent[b] = a for a matched pair, else -1.  TWO STATED
           SIMPLIFICATIONS: b's link to a later c is scored with b's OWN filter, not with the filter of the merged chain a -> b; and
           there is one pass, no iteration.
  relabel  root[i] = the head of i's chain; stitch_id[j, r] = root[track_id[j, r]] for an id within 0 .. N - 1, any other value (-1)
           stays.  A root's tables: first = the head's, last = the tail's, length = the sum over the chain, gaps = the sum over the
           chain + the number of links (a link is a gap); an id merged away gets -1 / -1 / 0 / 0; the rows from N on are copied.  Ids
           are NOT compacted: n_ids stays F T for the metrics.
Outputs, every element written: stitch_id [T, R] int32; stitch_parent, stitch_root [S, 32] int32 (-1 from N on); stitch_d2,
stitch_affinity [S, 32] fp32 (float32(d2) and float32(aff) of the link INTO b, 0 without one); stitch_first, stitch_last,
stitch_length, stitch_gaps [S, F T]; num_links [S]; stitch_status [S]: 0 stitched, 1 OVERFLOW.  OVERFLOW (N > 32: the solver has 32
columns): the sequence passes through -- ids and tables are bit copies, no link, parent -1 and root[i] = i for i < 32.  EXACT
CONSEQUENCES:
  1. with no admissible pair (a gate of 1e-300; max_gap below every gap) stitch_id and the four tables are the tracker's bit for bit.
  2. stitching is idempotent on ids in ONE case only: stitching the stitched output (ids relabelled, tables as written) links nothing
     new provided every chain had one link fewer than max_gap allows -- otherwise the merged track's own filter, which has seen both
     halves, may reach a fragment the halves' filters did not.  Nothing more is claimed.
Out of scope: a TrajectorySmoother behind a stitcher (its completed table assumes that a track spanning a frame was seen within max_age
frames of it: trajectory.completed_rows), stitching on a stream, more than 32 tracks per sequence.  max_gap = 8 and the chi-squared
gate are provisional like every other association default: UNMEASURED on a trained model (profiles/track_stitch.txt says what was
measured: the cost of the launch).

`SequenceTracker` owns no engine, like tile.TiledSceneParser and score.ParseScorer: it binds to a parse.SceneParser, refine.ParseRefiner,
prune.ParsePruner, propose.ParseProposer or tile.TiledSceneParser at R = S F rows, runs that provider's own `parse()` on the frames and
then, on the same engine stream, its own launch list of libair_hip.so entries (include/air_hip.h), ONE hipGraph after `capture()`
whatever F is -- the frames are walked inside air_track_associate:

  air_track_associate   the rule above (air_track_associate_optimal with matching="optimal", air_track_associate_motion with motion=,
                        which also reads the provider's `where` rows, air_track_associate_motion_gated with motion_gate= on top: the
                        same launch list otherwise);
  air_track_owner       track_owner[r, y, x] (int16) = the track id of the step that owns the pixel, -1 for background.

A particle_parse.ParticleParser is refused, with tile.TiledSceneParser's wording: its `parse()` takes no counts and its rows are particles
of an image, and the buffers the tracker reads next to the `what` rows (`boxes`, `score`, `num_objects`, `owner`) are the selected
particle's only behind a pruner or proposer -- bind one of those, they bind as every other provider.

Streams (`StreamTracker`; air_track_associate_stream, air_track_score_stream).  SequenceTracker is bound to n_frames = F and starts every
call with an empty table: a video longer than F, a live loop and sequences of different lengths need state that outlives a call.  A
STREAM is S sequences fed in CHUNKS of the tracker's F frames; a chunk carries valid[s] in 0..F frames of sequence s (rows s F + f with
f < valid[s]; the rows behind them are padding whose contents do not matter); the global index of a frame is frames_seen[s] + f.  CHUNK
INVARIANCE: feeding a sequence in any chunking -- ragged valid, valid = 0 included -- gives exactly the result of steps 1-5 (3' for
matching="optimal") on the concatenation of its valid frames: the same track_id, obj_state, prev_slot and affinity bits, prev_frame as
the GLOBAL frame index, the same first / last / length / gaps per track.  The carried state is device memory the kernel reads and
writes in place (include/air_hip.h states the layout; `new_stream_state` builds it in numpy): per sequence frames_seen and next_id,
per slot live, id, age, length, gaps, first, the last sighting's global frame and slot, its box and a BIT COPY of its `what` row.  The
tracks retired in a chunk come as a list (ascending retirement frame, then slot), the live ones stay in the state.  A stream issues
the ids 0..32766 (track_owner is int16); a birth beyond is OVERFLOW.  The metric continues across chunks: map[g], tracked[g],
present[g], the counters and sum_iou are carried, seq_counts and seq_iou are cumulative.  Out of scope on a stream: IDF1 (its overlap
table is indexed by global id: 1 MB per sequence at 32767 ids), HOTA (its tables are indexed by global id too, 19 thresholds deep:
StreamTracker has no `hota`), MOTS (the carried score state has a fixed layout: StreamTracker has no `mots`), ids beyond 32766
without `reset`, more than 32 live tracks.  Trajectories
on a stream are trajectory.StreamSmoother's: fixed-lag smoothed rows `lag` frames late and a forecast per chunk.  `reference_associate_stream` / `reference_score_stream` restate a chunk in numpy
with the per-frame code of the one-shot references.

The defaults of iou_gate, appearance_weight, birth_score and max_age are provisional: UNMEASURED on a trained model (profiles/track.txt
says what was measured); how often the optimal and the greedy matching differ on the parses of a trained model, and what that does to
IDF1, is unmeasured too (profiles/track_optimal.txt).  `reference_associate`, `reference_score` and `reference_identity` restate the
rules in numpy float64, `solve_assignment` the solver in Python integers.
"""
import math
from collections import OrderedDict
from typing import Dict

from .launch import destroy_graphs
from .stage import BoundStage
from .tile import TiledSceneParser, box_iou

MAX_SLOTS = 32                     # PARSE_MAXT / SCORE_MAXT: objects per frame and live tracks per sequence
MAX_GT = 8                         # SCORE_MAXG
MAX_IDS = 32767                    # F * T: an id fits int16
ABSENT, MATCHED, BORN, UNCONFIRMED, OVERFLOW, NONFINITE = range(6)
STATES = ("absent", "matched", "born", "unconfirmed", "overflow", "nonfinite")
COUNTS = ("gt", "matches", "misses", "fp", "idsw", "mostly_tracked", "mostly_lost", "gt_objects")
IDF_COUNTS = ("idtp", "gt_frames", "hyp_frames", "ids_with_overlap")
HOTA_ALPHAS = tuple(k / 20.0 for k in range(1, 20))               # the 19 localisation thresholds 0.05 .. 0.95
HOTA_COUNTS = ("tp", "fn", "fp")                                   # seq_hota_i [S, 19, 3]
HOTA_SUMS = ("ass", "ass_re", "ass_pr", "loc")                     # seq_hota_f [S, 19, 4]
HOTA_EPS = 2.0 ** -52                                              # pass 1 adds sim / d only where d > HOTA_EPS
MOTS_COUNTS = ("gt", "tp", "fn", "fp", "ids", "mostly_tracked", "mostly_lost", "gt_objects")      # seq_mots_i [S, 8]
MOTS_OUTPUTS = ("seq_mots_i", "seq_mots_f", "mots_match", "mots_iou")
MOTS_NEEDS_INSTANCES = "mots=True scores the tracks as masks: it needs gt_instances [S, F, H, W] (int8, -1 = background)"
MATCHINGS = ("greedy", "optimal")
PROFIT_SCALE = 4294967296.0        # 2^32: profit = 1 + floor(aff * 2^32)
DEFAULTS = dict(iou_gate=0.1, appearance_weight=0.25, birth_score=0.5, max_age=1)
MOTION_GATE_DEFAULT = 13.2767       # motion_gate=True: the 0.99 quantile of chi-squared with 4 degrees of freedom (provisional)
MOTION_ON_A_STREAM = ("motion is out of scope on a stream: the state carried between chunks would need each slot's filter state (14 "
                      "doubles); track the sequence in one call with SequenceTracker(motion=...) (motion_gate= goes with motion=)")


def check_arguments(max_steps, n_frames, n_rows=None, iou_gate=0.1, appearance_weight=0.25, birth_score=0.5, max_age=1,
                    matching="greedy"):
    """Refuse what air_track_associate refuses (pure host code: importable and callable without a GPU).  Returns (T, F, S) with S = None
    when `n_rows` is not given."""
    gate, w, birth = float(iou_gate), float(appearance_weight), float(birth_score)
    if not (math.isfinite(gate) and 0.0 <= gate < 1.0):
        raise ValueError("iou_gate must be a number within [0, 1), got %r" % (iou_gate,))
    if not (math.isfinite(w) and 0.0 <= w <= 1.0):
        raise ValueError("appearance_weight must be a number within [0, 1], got %r" % (appearance_weight,))
    if not (math.isfinite(birth) and 0.0 <= birth <= 1.0):
        raise ValueError("birth_score must be a number within [0, 1], got %r" % (birth_score,))
    if isinstance(max_age, bool) or int(max_age) != max_age or int(max_age) < 0:
        raise ValueError("max_age must be an integer >= 0, got %r" % (max_age,))
    if matching not in MATCHINGS:
        raise ValueError("matching must be one of %s, got %r" % (" / ".join(repr(m) for m in MATCHINGS), matching))
    T, F = int(max_steps), int(n_frames)
    if not 1 <= T <= MAX_SLOTS:
        raise ValueError("max_steps must be within 1..%d, got %d" % (MAX_SLOTS, T))
    if int(n_frames) != n_frames or F < 1:
        raise ValueError("n_frames must be an integer >= 1, got %r" % (n_frames,))
    if F * T > MAX_IDS:
        raise ValueError("%d frames of %d steps could issue %d track ids; an id must fit int16: at most %d" % (F, T, F * T, MAX_IDS))
    S = None
    if n_rows is not None:
        if int(n_rows) < 1 or int(n_rows) % F:
            raise ValueError("the provider's %d rows are no multiple of %d frames" % (int(n_rows), F))
        S = int(n_rows) // F
    return T, F, S


def _sequential_sum(x):
    """the sum over the last axis added in ascending index order (np.sum adds pairwise)"""
    import numpy as np
    return np.cumsum(x, axis=-1)[..., -1]


def solve_assignment(profit, admissible):
    """The solver of air_track_associate_optimal restated in Python integers.  profit [n, m] (int64), admissible [n, m] (bool): row i
    may take an admissible column c for profit[i, c] or stay unmatched for 0 (its own column m + i).  Returns col [n] (int64): the
    column of row i, -1 for unmatched -- the one-to-one assignment of the largest summed profit, and among several of them the one
    this procedure yields (the module text states it): rows inserted in ascending order; from the inserted row the alternating tree
    grows by the unused column of the least reduced cost minv, the lowest column among equal values, a column keeping the first tree
    column that gave it that cost (`way`); at a free column the rows along the path move one column on."""
    import numpy as np
    profit, admissible = np.asarray(profit).astype(np.int64), np.asarray(admissible).astype(bool)
    n, m = profit.shape
    C = m + n
    NONE = C                                                       # the virtual column an insertion starts from
    u, v, row = [0] * n, [0] * C, [-1] * C
    for i in range(n):
        minv, way, used, in_tree = [None] * C, [NONE] * C, [False] * C, [False] * n
        j0, i0 = NONE, i
        while True:
            if j0 != NONE:
                used[j0] = True
            in_tree[i0] = True
            for c in range(C):
                if used[c] or not (admissible[i0, c] if c < m else c - m == i0):
                    continue
                cur = -(int(profit[i0, c]) if c < m else 0) - u[i0] - v[c]
                if minv[c] is None or cur < minv[c]:
                    minv[c], way[c] = cur, j0
            delta, j1 = min((minv[c], c) for c in range(C) if not used[c] and minv[c] is not None)      # (row i0's own column is open)
            for r in range(n):
                if in_tree[r]:
                    u[r] += delta
            for c in range(C):
                if used[c]:
                    v[c] -= delta
                elif minv[c] is not None:
                    minv[c] -= delta
            j0, i0 = j1, row[j1]
            if i0 < 0:
                break
        while j0 != NONE:
            j1 = way[j0]
            row[j0] = i if j1 == NONE else row[j1]
            j0 = j1
    col = np.full(n, -1, np.int64)
    for c in range(m):
        if row[c] >= 0:
            col[row[c]] = c
    return col


def check_motion(motion):
    """motion=None / False (off), True (trajectory.DEFAULTS) or a dict with any of process_noise, measurement_noise, velocity_var (the
    rest: the defaults) -> None or the complete dict, its noise terms inside the smoother's supported domain (trajectory.check_arguments
    raises its own messages outside it)"""
    if motion is None or motion is False:
        return None
    from . import trajectory                                       # (lazily: trajectory imports this module)
    terms = dict(trajectory.DEFAULTS)
    if motion is not True:
        if not isinstance(motion, dict):
            raise ValueError("motion must be None, True or a dict with any of %s, got %r" % (", ".join(terms), motion))
        unknown = sorted(set(motion) - set(terms), key=str)
        if unknown:
            raise ValueError("motion: unknown keys %r; it takes %s" % (unknown, ", ".join(terms)))
        terms.update(motion)
    q, r, vv = trajectory.check_arguments(1, 1, **terms)[5:]
    return dict(process_noise=q, measurement_noise=r, velocity_var=vv)


def check_motion_gate(motion_gate, motion=None):
    """motion_gate=None / False (off), True (MOTION_GATE_DEFAULT) or a finite number > 0: a squared Mahalanobis distance -> None or the
    float.  A gate needs the filter whose covariance it reads: without motion (None / False) it raises."""
    if motion_gate is None or motion_gate is False:
        return None
    if motion is None or motion is False:
        raise ValueError("motion_gate gates on the covariance of the motion filter: it needs motion=True or motion=dict(...)")
    if motion_gate is True:
        return MOTION_GATE_DEFAULT
    try:
        gate = float(motion_gate)
    except (TypeError, ValueError):
        gate = float("nan")
    if not (math.isfinite(gate) and gate > 0.0):
        raise ValueError("motion_gate must be None, True or a finite squared Mahalanobis distance > 0, got %r" % (motion_gate,))
    return gate


def _motion_predicted_state(filt, m, q, r):
    """the gate's step 2, per track: (xp [4], s [4]) of the filter m frames after its last sighting -- the m - 1 frames coasted over
    predicted one by one, then the predicted tuple of one more trajectory._filter_step (never m v); s = Pxx- + r per component (the
    two scales share one value, the two shifts another)"""
    from .trajectory import _filter_step
    for _ in range(m - 1):
        filt = _filter_step(filt, None, q, r)[1]
    pred = _filter_step(filt, None, q, r)[0]
    return pred[0], pred[2] + r


def _motion_d2(xp, s, z):
    """the gate's step 2, per pair: the squared Mahalanobis distance of the sighting z from the predicted state, summed in the order
    [sx, tx, sy, ty]: each term one product and one quotient"""
    e = z - xp
    return ((e[0] * e[0] / s[0] + e[1] * e[1] / s[1]) + e[2] * e[2] / s[2]) + e[3] * e[3] / s[3]


def _gated_pair(d2, msd, w, gate, pred_box, box):
    """the gate's step 2, per pair: None for an inadmissible pair (d2 <= gate fails, as it does for a NaN or an inf), else the affinity:
    rational in d2 and msd, within [0, 1].  pred_box and box are NOT read -- iou_gate is not applied under the gate; they are passed so
    that a test can plant a rule that does read them"""
    if not d2 <= gate:
        return None
    return (1.0 - w) / (1.0 + d2) + w / (1.0 + msd)


def _motion_predict(filt, m, last_box, img_size):
    """step 2 with motion: (pred_where, pred_box) of a track m frames after its last sighting, from its filtered state there --
    trajectory._forecast_where's row and its scene box in fp32; a box that is not finite falls back to the last-sighting box"""
    import numpy as np
    from .tile import scene_boxes
    from .trajectory import _forecast_where
    with np.errstate(all="ignore"):
        pred_where = _forecast_where(filt[0], filt[1], m)
        pred_box = scene_boxes(pred_where, img_size)
    return pred_where, (pred_box if np.isfinite(pred_box).all() else last_box.copy())


def _motion_advance(filt, m, z, q, r):
    """booking a match with motion: the filtered state m frames on -- the m - 1 frames coasted over predicted one by one, then the
    step with the sighting z (trajectory._filter_step, verbatim)"""
    from .trajectory import _filter_step
    for _ in range(m - 1):
        filt = _filter_step(filt, None, q, r)[1]
    return _filter_step(filt, z, q, r)[1]


def _associate_frame(live, next_id, fg, what, boxes, score, n, rule, margins, id_limit=None, motion=None):
    """Steps 1-5 of the rule on ONE frame (the code reference_associate and reference_associate_stream share).  live: slot -> dict(id,
    f, j, age, length, gaps, first, box, what) with the last sighting's box [4] and what row [A] as fp32 copies; fg: the frame's index
    (in the stream); what [T, A], boxes [T, 4], score [T]: the frame's fp32 rows; n: its clipped count; rule = (gate, w, birth,
    max_age, matching); margins: [gate_margin, round_margin], updated in place; id_limit: a birth at next_id == id_limit is OVERFLOW.
    motion: None, or dict(where [T, 4] fp32, img_size, q [4], r, vv, pred_where [T, 4], pred_boxes [T, 4] (written)): the rule of
    reference_associate_motion, a track then carries `filt`, its filtered state at the last sighting.  With motion["gate"] = G (and
    pred_d2 [T], written) the pairs are gated and ranked by their squared Mahalanobis distance; margins[0] is then min |d2 - G|.
    Returns (state, ids, affinity, prev_frame, prev_slot, next_id, born [tracks], retired [(slot, track)] in ascending slot)."""
    import numpy as np
    gate, w, birth, max_age, matching = rule
    T, A = what.shape
    state = np.zeros(T, np.int64)
    ids, pf, ps, aff32 = np.full(T, -1, np.int32), np.full(T, -1, np.int32), np.full(T, -1, np.int32), np.zeros(T, np.float32)
    what64 = what.astype(np.float64)
    finite = []
    for j in range(n):                                             # 1. states
        ok = np.isfinite(boxes[j]).all() and np.isfinite(score[j]) and np.isfinite(what[j]).all()
        ok = ok and (motion is None or np.isfinite(motion["where"][j]).all())
        state[j] = UNCONFIRMED if ok else NONFINITE                # (finite and open: settled below)
        if ok:
            finite.append(j)
    aff = {}                                                       # 2. affinity of the admissible pairs
    pred = {}                                                      # motion: slot -> (pred_where, pred_box)
    G = None if motion is None else motion.get("gate")
    d2s = {}                                                       # the gate: (slot, j) -> d2 of an admissible pair
    for k, t in live.items():
        if not finite:
            break
        d = t["what"].astype(np.float64)[None, :] - what64[finite]
        msd = _sequential_sum(d * d) / np.float64(A)
        if motion is not None:
            pred[k] = _motion_predict(t["filt"], fg - t["f"], t["box"], motion["img_size"])
        if G is not None:
            with np.errstate(all="ignore"):
                xp, s_in = _motion_predicted_state(t["filt"], fg - t["f"], motion["q"], motion["r"])
        for q, j in enumerate(finite):
            if G is not None:                                      # the Mahalanobis gate: iou_gate is not applied
                with np.errstate(all="ignore"):
                    d2 = float(_motion_d2(xp, s_in, motion["where"][j].astype(np.float64)))
                    margins[0] = min(margins[0], abs(d2 - G))
                    v = _gated_pair(d2, float(msd[q]), w, G, pred[k][1], boxes[j])
                if v is not None:
                    aff[(k, j)], d2s[(k, j)] = v, d2
                continue
            iou = box_iou(t["box"] if motion is None else pred[k][1], boxes[j])
            margins[0] = min(margins[0], abs(iou - gate))
            if iou > gate:
                aff[(k, j)] = (1.0 - w) * iou + w / (1.0 + float(msd[q]))

    def matched(k, j):
        t = live[k]
        state[j] = MATCHED
        ids[j], pf[j], ps[j] = t["id"], t["f"], t["j"]
        aff32[j] = np.float32(aff[(k, j)])
        if motion is not None:
            motion["pred_where"][j], motion["pred_boxes"][j] = pred[k]
            if G is not None:
                motion["pred_d2"][j] = np.float32(d2s[(k, j)])
            with np.errstate(all="ignore"):
                t["filt"] = _motion_advance(t["filt"], fg - t["f"], motion["where"][j].astype(np.float64), motion["q"], motion["r"])
        t["gaps"] += 1 if t["age"] > 0 else 0
        t["age"], t["length"], t["f"], t["j"] = 0, t["length"] + 1, fg, j
        t["box"], t["what"] = boxes[j].copy(), what[j].copy()

    if matching == "optimal" and aff:                              # 3. the optimal assignment
        profit, admissible = np.zeros((len(finite), MAX_SLOTS), np.int64), np.zeros((len(finite), MAX_SLOTS), bool)
        for (k, j), v in aff.items():
            profit[finite.index(j), k], admissible[finite.index(j), k] = 1 + int(math.floor(v * PROFIT_SCALE)), True
        for q, k in enumerate(solve_assignment(profit, admissible)):
            if k >= 0:
                matched(int(k), finite[q])
        aff = {}
    while aff:                                                     # 3. greedy matching
        ranked = sorted(aff, key=lambda kj: (-aff[kj], live[kj[0]]["id"], kj[1]))
        k, j = ranked[0]
        if len(ranked) > 1:
            margins[1] = min(margins[1], aff[ranked[0]] - aff[ranked[1]])
        matched(k, j)
        aff = {kj: v for kj, v in aff.items() if kj[0] != k and kj[1] != j}
    born = []
    for j in finite:                                               # 4. births
        if state[j] != UNCONFIRMED or not float(score[j]) >= birth:
            continue
        free = [k for k in range(MAX_SLOTS) if k not in live]
        if not free or (id_limit is not None and next_id >= id_limit):
            state[j] = OVERFLOW
            continue
        state[j] = BORN
        live[free[0]] = dict(id=next_id, f=fg, j=j, age=0, length=1, gaps=0, first=fg, box=boxes[j].copy(), what=what[j].copy())
        if motion is not None:
            from .trajectory import _filter_start
            live[free[0]]["filt"] = _filter_start(motion["where"][j].astype(np.float64), motion["r"], motion["vv"])
        born.append(live[free[0]])
        ids[j] = next_id
        next_id += 1
    retired = []
    for k in sorted(live):                                         # 5. ageing
        t = live[k]
        if t["f"] != fg:
            t["age"] += 1
            if t["age"] > max_age:
                retired.append((k, live.pop(k)))
    return state, ids, aff32, pf, ps, next_id, born, retired


def reference_associate(what, boxes, score, num_objects, n_frames, iou_gate=0.1, appearance_weight=0.25, birth_score=0.5, max_age=1,
                        return_margins=False, matching="greedy"):
    """air_track_associate restated in numpy float64.  Arrays as the kernel takes them: what [T, R, A], boxes [T, R, 4], score [T, R]
    (fp32), num_objects [R], R = S * n_frames.  Returns track_id [T, R] int32, obj_state [T, R] int8, affinity [T, R] float32,
    prev_frame, prev_slot [T, R] int32, num_tracks [S] int32, track_first, track_last, track_length, track_gaps [S, F * T] int32,
    state_counts [S, 6] int32.  return_margins=True adds how far the decisions are from flipping, per sequence: gate_margin [S] (the
    smallest |iou - iou_gate| over the pairs of step 2), round_margin [S] (the smallest aff(winner) - aff(runner-up) over the greedy
    rounds with more than one open admissible pair; inf without any).  matching="optimal": air_track_associate_optimal, step 3 by
    `solve_assignment`; return_margins then adds gate_margin only (there are no greedy rounds)."""
    return _associate_sequences(what, boxes, score, num_objects, n_frames, iou_gate, appearance_weight, birth_score, max_age,
                                return_margins, matching)


def _associate_sequences(what, boxes, score, num_objects, n_frames, iou_gate, appearance_weight, birth_score, max_age, return_margins,
                         matching, motion=None):
    """the body of reference_associate and reference_associate_motion (motion: None, or dict(where [T, R, 4], img_size, q [4], r,
    vv, return_state))"""
    import numpy as np
    what, boxes, score = (np.asarray(a, np.float32) for a in (what, boxes, score))
    n_in = np.asarray(num_objects).astype(np.int64)
    T, R, A = what.shape
    T, F, S = check_arguments(T, n_frames, R, iou_gate, appearance_weight, birth_score, max_age, matching)
    rule = (float(iou_gate), float(appearance_weight), float(birth_score), int(max_age), matching)
    FT = F * T
    out = {"track_id": np.full((T, R), -1, np.int32), "obj_state": np.zeros((T, R), np.int8), "affinity": np.zeros((T, R), np.float32),
           "prev_frame": np.full((T, R), -1, np.int32), "prev_slot": np.full((T, R), -1, np.int32), "num_tracks": np.zeros(S, np.int32),
           "track_first": np.full((S, FT), -1, np.int32), "track_last": np.full((S, FT), -1, np.int32),
           "track_length": np.zeros((S, FT), np.int32), "track_gaps": np.zeros((S, FT), np.int32),
           "state_counts": np.zeros((S, 6), np.int32)}
    if motion is not None:
        out.update(pred_where=np.zeros((T, R, 4), np.float32), pred_boxes=np.zeros((T, R, 4), np.float32))
        if motion.get("gate") is not None:
            out.update(pred_d2=np.zeros((T, R), np.float32))
        if motion["return_state"]:
            out["motion_state"] = {}
    gate_margin, round_margin = np.full(S, np.inf), np.full(S, np.inf)
    for s in range(S):
        live = {}                                                  # slot -> the track
        next_id = 0
        margins = [np.inf, np.inf]

        def retire(t):
            out["track_last"][s, t["id"]], out["track_length"][s, t["id"]], out["track_gaps"][s, t["id"]] = t["f"], t["length"], t["gaps"]
            if motion is not None and motion["return_state"]:
                out["motion_state"][(s, t["id"])] = t["filt"]

        for f in range(F):
            r = s * F + f
            n = int(min(max(n_in[r], 0), T))
            frame_motion = None
            if motion is not None:
                frame_motion = dict(motion, where=motion["where"][:, r], pred_where=out["pred_where"][:, r],
                                    pred_boxes=out["pred_boxes"][:, r])
                if "pred_d2" in out:
                    frame_motion.update(pred_d2=out["pred_d2"][:, r])
            state, ids, aff32, pf, ps, next_id, born, retired = _associate_frame(live, next_id, f, what[:, r], boxes[:, r], score[:, r],
                                                                                 n, rule, margins, motion=frame_motion)
            for t in born:
                out["track_first"][s, t["id"]] = f
            for _, t in retired:
                retire(t)
            out["track_id"][:, r], out["affinity"][:, r], out["prev_frame"][:, r], out["prev_slot"][:, r] = ids, aff32, pf, ps
            out["obj_state"][:, r] = state
            out["state_counts"][s] += np.bincount(state, minlength=6).astype(np.int32)
        for k in sorted(live):
            retire(live[k])
        out["num_tracks"][s] = next_id
        gate_margin[s], round_margin[s] = margins
    if return_margins:
        out["gate_margin"] = gate_margin
        if matching == "greedy":
            out["round_margin"] = round_margin
    return out


def reference_associate_motion(what, where, boxes, score, num_objects, n_frames, img_size, iou_gate=0.1, appearance_weight=0.25,
                               birth_score=0.5, max_age=1, matching="greedy", process_noise=None, measurement_noise=None,
                               velocity_var=None, return_margins=False, return_state=False, gate=None):
    """air_track_associate_motion restated in numpy float64 (MOTION in the module text): reference_associate's arrays and rule
    arguments, where [T, R, 4] fp32 = [sx, tx, sy, ty], img_size (H, W), and the noise terms of the trajectory filter (None: trajectory.
    DEFAULTS; outside the supported domain: trajectory.check_arguments' messages).  Returns reference_associate's outputs (matching=
    "optimal": air_track_associate_optimal's step 3) and pred_where, pred_boxes [T, R, 4] float32: for a MATCHED object the prediction
    of its track that the match was made against, zero otherwise.  return_margins as in reference_associate (gate_margin over the IoUs
    with the PREDICTED boxes).  return_state=True adds motion_state: (s, id) -> the filtered state (x, v, Pxx, Pxv, Pvv), float64 [4]
    each over [sx, tx, sy, ty], of every track at its last sighting.  gate=G (None: off; True: MOTION_GATE_DEFAULT):
    air_track_associate_motion_gated -- the pairs gated by d2 <= G and ranked by (1 - w) / (1 + d2) + w / (1 + msd), iou_gate not applied;
    adds pred_d2 [T, R] float32 (the d2 of the pair a MATCHED object was matched in, zero otherwise), and gate_margin is then the
    smallest |d2 - G|."""
    import numpy as np
    gate = check_motion_gate(gate, True)
    terms = {k: v for k, v in dict(process_noise=process_noise, measurement_noise=measurement_noise, velocity_var=velocity_var).items()
             if v is not None}
    terms = check_motion(terms or True)
    (q_shift, q_scale), H, W = terms["process_noise"], int(img_size[0]), int(img_size[1])
    if H < 1 or W < 1:
        raise ValueError("img_size must be (H, W) with H, W >= 1, got %r" % (img_size,))
    where = np.asarray(where, np.float32)
    if where.shape != tuple(np.shape(what)[:2]) + (4,):
        raise ValueError("where: expected %s, got %s" % (tuple(np.shape(what)[:2]) + (4,), where.shape))
    motion = dict(where=where, img_size=(H, W), q=np.array([q_scale, q_shift, q_scale, q_shift], np.float64),
                  r=terms["measurement_noise"], vv=terms["velocity_var"], return_state=bool(return_state), gate=gate)
    return _associate_sequences(what, boxes, score, num_objects, n_frames, iou_gate, appearance_weight, birth_score, max_age,
                                return_margins, matching, motion)


# ---- streams: the state that outlives a call (include/air_hip.h states the layout) -------------------------------------------------------
ST_LIVE, ST_ID, ST_AGE, ST_LENGTH, ST_GAPS, ST_FIRST, ST_LAST_FRAME, ST_LAST_SLOT = range(8)
ST_FIELDS = ("live", "id", "age", "length", "gaps", "first", "last_frame", "last_slot")
ST_EMPTY = (0, -1, 0, 0, 0, -1, -1, -1)                            # a slot that is not live, field by field (box and what: 0)
STATE_KEYS = ("seq", "slots", "box", "what")
SCORE_STATE_KEYS = ("score_i", "score_f")
RETIRED = ("retired_id", "retired_first", "retired_last", "retired_length", "retired_gaps")
STREAM_OUTPUTS = ("track_id", "obj_state", "affinity", "prev_frame", "prev_slot", "state_counts", "num_retired") + RETIRED
MAX_FRAMES_SEEN = 2 ** 31 - 1


def new_stream_state(n_sequences, what_size):
    """the state of a stream that has seen nothing, as numpy arrays: seq [S, 2] int32 {frames_seen, next_id}, slots [S, 8, 32] int32
    (ST_FIELDS), box [S, 32, 4] and what [S, 32, A] fp32"""
    import numpy as np
    S, A = int(n_sequences), int(what_size)
    slots = np.empty((S, 8, MAX_SLOTS), np.int32)
    slots[:] = np.asarray(ST_EMPTY, np.int32)[None, :, None]
    return {"seq": np.zeros((S, 2), np.int32), "slots": slots, "box": np.zeros((S, MAX_SLOTS, 4), np.float32),
            "what": np.zeros((S, MAX_SLOTS, A), np.float32)}


def new_score_state(n_sequences):
    """score_i [S, 32] int32 = {gt, matches, misses, fp, idsw, 0, 0, 0, map[8] (-1), tracked[8], present[8]}, score_f [S] float64"""
    import numpy as np
    si = np.zeros((int(n_sequences), 32), np.int32)
    si[:, 8:16] = -1
    return {"score_i": si, "score_f": np.zeros(int(n_sequences), np.float64)}


def stream_live(state):
    """the live tracks of a stream state, per sequence a list (ascending slot) of dict(slot, id, first, last, length, gaps, age)"""
    import numpy as np
    sl = np.asarray(state["slots"])
    return [[dict(slot=k, id=int(q[ST_ID, k]), first=int(q[ST_FIRST, k]), last=int(q[ST_LAST_FRAME, k]), length=int(q[ST_LENGTH, k]),
                  gaps=int(q[ST_GAPS, k]), age=int(q[ST_AGE, k])) for k in range(MAX_SLOTS) if q[ST_LIVE, k]] for q in sl]


def check_valid(valid, n_sequences, n_frames):
    """valid=None (every frame of the chunk) or [S] integers -> int64 [S] clipped to 0..F as the kernel clips it"""
    import numpy as np
    S, F = int(n_sequences), int(n_frames)
    if valid is None:
        return np.full(S, F, np.int64)
    v = np.asarray(valid)
    if v.shape != (S,) or not np.issubdtype(v.dtype, np.integer):
        raise ValueError("valid: expected %d integers (the frames of each sequence in this chunk), got shape %s %s"
                         % (S, tuple(v.shape), v.dtype))
    return np.clip(v.astype(np.int64), 0, F)


def check_frames_seen(frames_seen, valid):
    """refuse a chunk that would take a sequence's global frame index past int32"""
    import numpy as np
    after = np.asarray(frames_seen, np.int64) + np.asarray(valid, np.int64)
    if (after > MAX_FRAMES_SEEN).any():
        s = int(np.argmax(after))
        raise ValueError("frames_seen of sequence %d would reach %d; the global frame index must fit int32: reset() the sequence"
                         % (s, int(after[s])))
    return after


def reference_associate_stream(state, what, boxes, score, num_objects, n_frames, valid=None, iou_gate=0.1, appearance_weight=0.25,
                               birth_score=0.5, max_age=1, matching="greedy", return_margins=False):
    """air_track_associate_stream restated in numpy float64, with reference_associate's per-frame code: ONE chunk.  state: None
    (a stream starts) or what an earlier call returned (it is not modified); the arrays as the kernel takes them, R = S * n_frames;
    valid [S] (None: every frame).  Returns (outputs, state): track_id, obj_state, affinity, prev_frame (GLOBAL), prev_slot [T, R]
    with -1 / ABSENT / 0 / -1 / -1 on padding rows, state_counts [S, 6] (valid frames), num_retired [S], retired_id / _first / _last /
    _length / _gaps [S, 32 + F * T] (ascending retirement frame, then slot; unused rows -1 / -1 / -1 / 0 / 0); and the new state
    (new_stream_state's arrays).  Ids: 0..32766, a birth beyond is OVERFLOW.  return_margins as in reference_associate."""
    import numpy as np
    what, boxes, score = (np.asarray(a, np.float32) for a in (what, boxes, score))
    n_in = np.asarray(num_objects).astype(np.int64)
    T, R, A = what.shape
    T, F, S = check_arguments(T, n_frames, R, iou_gate, appearance_weight, birth_score, max_age, matching)
    rule = (float(iou_gate), float(appearance_weight), float(birth_score), int(max_age), matching)
    v_in = check_valid(valid, S, F)
    state = new_stream_state(S, A) if state is None else {k: np.array(state[k]) for k in STATE_KEYS}
    if state["what"].shape != (S, MAX_SLOTS, A) or state["seq"].shape != (S, 2):
        raise ValueError("the state is one of %s sequences with what rows of %d values, the chunk has %d and %d"
                         % (state["seq"].shape[0], state["what"].shape[-1], S, A))
    check_frames_seen(state["seq"][:, 0], v_in)
    cap = MAX_SLOTS + F * T
    out = {"track_id": np.full((T, R), -1, np.int32), "obj_state": np.zeros((T, R), np.int8), "affinity": np.zeros((T, R), np.float32),
           "prev_frame": np.full((T, R), -1, np.int32), "prev_slot": np.full((T, R), -1, np.int32),
           "state_counts": np.zeros((S, 6), np.int32), "num_retired": np.zeros(S, np.int32)}
    out.update({k: np.full((S, cap), -1 if k in RETIRED[:3] else 0, np.int32) for k in RETIRED})
    gate_margin, round_margin = np.full(S, np.inf), np.full(S, np.inf)
    for s in range(S):
        sl = state["slots"][s]
        live = {k: dict(id=int(sl[ST_ID, k]), f=int(sl[ST_LAST_FRAME, k]), j=int(sl[ST_LAST_SLOT, k]), age=int(sl[ST_AGE, k]),
                        length=int(sl[ST_LENGTH, k]), gaps=int(sl[ST_GAPS, k]), first=int(sl[ST_FIRST, k]),
                        box=state["box"][s, k].copy(), what=state["what"][s, k].copy()) for k in range(MAX_SLOTS) if sl[ST_LIVE, k]}
        base, next_id = int(state["seq"][s, 0]), int(state["seq"][s, 1])
        margins = [np.inf, np.inf]
        n_ret = 0
        for f in range(int(v_in[s])):
            r = s * F + f
            n = int(min(max(n_in[r], 0), T))
            st, ids, aff32, pf, ps, next_id, _, retired = _associate_frame(live, next_id, base + f, what[:, r], boxes[:, r], score[:, r],
                                                                           n, rule, margins, MAX_IDS)
            for _, t in retired:
                for key, val in zip(RETIRED, (t["id"], t["first"], t["f"], t["length"], t["gaps"])):
                    out[key][s, n_ret] = val
                n_ret += 1
            out["track_id"][:, r], out["affinity"][:, r], out["prev_frame"][:, r], out["prev_slot"][:, r] = ids, aff32, pf, ps
            out["obj_state"][:, r] = st
            out["state_counts"][s] += np.bincount(st, minlength=6).astype(np.int32)
        out["num_retired"][s] = n_ret
        state["seq"][s] = (base + int(v_in[s]), next_id)
        sl[:] = np.asarray(ST_EMPTY, np.int32)[:, None]
        state["box"][s], state["what"][s] = 0, 0
        for k, t in live.items():
            sl[:, k] = (1, t["id"], t["age"], t["length"], t["gaps"], t["first"], t["f"], t["j"])
            state["box"][s, k], state["what"][s, k] = t["box"], t["what"]
        gate_margin[s], round_margin[s] = margins
    if return_margins:
        out["gate_margin"] = gate_margin
        if matching == "greedy":
            out["round_margin"] = round_margin
    return out, state


def reset_stream_state(state, sequences=None):
    """restart all (None) or some sequences of a numpy stream state, in place (association and, if present, score keys)"""
    import numpy as np
    S = state["seq"].shape[0]
    rows = np.arange(S) if sequences is None else np.atleast_1d(np.asarray(sequences, np.int64))
    if rows.size and (rows.min() < 0 or rows.max() >= S):
        raise ValueError("reset: sequences within 0..%d, got %r" % (S - 1, sequences))
    fresh = new_stream_state(1, state["what"].shape[-1])
    for k in STATE_KEYS:
        state[k][rows] = fresh[k][0]
    if "score_i" in state:
        fs = new_score_state(1)
        state["score_i"][rows], state["score_f"][rows] = fs["score_i"][0], 0.0
    return state


def _score_frame(c, remembered, tracked, frames, sum_iou, boxes, ids, n, gt, tau):
    """One frame of the identity metric (the code reference_score and reference_score_stream share): boxes [T, 4], ids [T], gt [G, 4].
    c (the counters), remembered, tracked, frames are updated in place; returns (gt_match [G], sum_iou)."""
    import numpy as np
    G = gt.shape[0]
    gm = np.full(G, -1, np.int32)
    hyp = [j for j in range(n) if ids[j] >= 0 and np.isfinite(boxes[j]).all()]
    present = [g for g in range(G) if gt[g, 2] > 0]
    iou = {(g, j): box_iou(gt[g], boxes[j]) for g in present for j in hyp}
    match, taken = {}, set()
    for g in present:                                              # 1. the remembered track keeps its object
        if remembered[g] < 0:
            continue
        j = next((j for j in hyp if ids[j] == remembered[g] and iou[(g, j)] > tau), None)
        if j is not None and j not in taken:
            match[g] = j
            taken.add(j)
    while True:                                                    # 2. the rest greedily
        open_pairs = [(g, j) for (g, j), v in iou.items() if g not in match and j not in taken and v > tau]
        if not open_pairs:
            break
        g, j = min(open_pairs, key=lambda gj: (-iou[gj], gj[0], gj[1]))
        match[g] = j
        taken.add(j)
    for g in present:                                              # 3., 4.
        c["gt"] += 1
        frames[g] += 1
        if g not in match:
            c["misses"] += 1
            continue
        j = match[g]
        gm[g] = j
        c["matches"] += 1
        tracked[g] += 1
        sum_iou = sum_iou + iou[(g, j)]
        c["idsw"] += 1 if remembered[g] >= 0 and remembered[g] != ids[j] else 0
        remembered[g] = int(ids[j])
    c["fp"] += len(hyp) - len(taken)
    return gm, sum_iou


def _score_objects(c, tracked, frames):
    """mostly tracked / mostly lost / gt objects from the per-slot counts, into c"""
    c["gt_objects"] = c["mostly_tracked"] = c["mostly_lost"] = 0
    for g in range(len(frames)):
        if frames[g] > 0:
            c["gt_objects"] += 1
            c["mostly_tracked"] += 1 if 5 * tracked[g] >= 4 * frames[g] else 0
            c["mostly_lost"] += 1 if 5 * tracked[g] <= frames[g] else 0


def _score_arguments(boxes, num_objects, track_id, gt_boxes, n_frames, tau=None, n_ids=False, check_T=False):
    """the arguments of the scoring references, normalised and checked in one order: T (check_T: air_track_hota's), G, the frames, tau
    (None: the entry takes none), n_ids (False: the entry takes none and None comes back; None: n_frames * T)"""
    import numpy as np
    boxes = np.asarray(boxes, np.float32)
    gt = np.asarray(gt_boxes, np.float32)
    gt = gt.reshape(-1, gt.shape[-2], 4)
    ids, n_in = np.asarray(track_id).astype(np.int64), np.asarray(num_objects).astype(np.int64)
    T, R = ids.shape
    G, F = gt.shape[1], int(n_frames)
    if n_ids is not False:
        n_ids = F * T if n_ids is None else int(n_ids)
    if check_T and not 1 <= T <= MAX_SLOTS:
        raise ValueError("track_id: 1..%d objects per frame, got %d" % (MAX_SLOTS, T))
    if not 1 <= G <= MAX_GT:
        raise ValueError("gt_boxes: 1..%d ground-truth slots, got %d" % (MAX_GT, G))
    if F < 1 or R % F or gt.shape[0] != R:
        raise ValueError("%d rows / %d ground-truth rows are not sequences of %d frames" % (R, gt.shape[0], F))
    if tau is not None:
        tau = float(tau)
        if not 0.0 <= tau <= 1.0:
            raise ValueError("tau must be within [0, 1], got %r" % (tau,))
    if n_ids is not False and not 1 <= n_ids <= MAX_IDS:
        raise ValueError("n_ids must be within 1..%d, got %d" % (MAX_IDS, n_ids))
    return boxes, gt, ids, n_in, T, R, G, F, tau, (None if n_ids is False else n_ids)


def reference_score(boxes, num_objects, track_id, gt_boxes, n_frames, tau=0.5):
    """air_track_score restated in numpy float64.  boxes [T, R, 4], num_objects [R], track_id [T, R], gt_boxes [R, G, 4] (or
    [S, F, G, 4]).  Returns seq_counts [S, 8] int32 (COUNTS), seq_iou [S] float64, gt_match [R, G] int32."""
    import numpy as np
    boxes, gt, ids, n_in, T, R, G, F, tau, _ = _score_arguments(boxes, num_objects, track_id, gt_boxes, n_frames, tau)
    S = R // F
    counts, seq_iou, gt_match = np.zeros((S, 8), np.int32), np.zeros(S, np.float64), np.full((R, G), -1, np.int32)
    for s in range(S):
        remembered = [-1] * G
        tracked, frames = [0] * G, [0] * G
        c = dict.fromkeys(COUNTS, 0)
        for f in range(F):
            r = s * F + f
            n = int(min(max(n_in[r], 0), T))
            gt_match[r], seq_iou[s] = _score_frame(c, remembered, tracked, frames, seq_iou[s], boxes[:, r], ids[:, r], n, gt[r], tau)
        _score_objects(c, tracked, frames)
        counts[s] = [c[k] for k in COUNTS]
    return {"seq_counts": counts, "seq_iou": seq_iou, "gt_match": gt_match}


def reference_score_stream(state, boxes, num_objects, track_id, gt_boxes, n_frames, valid=None, tau=0.5):
    """air_track_score_stream restated in numpy float64, with reference_score's per-frame code: ONE chunk.  state: None (a stream
    starts) or what an earlier call returned (not modified): new_score_state's arrays.  Returns (outputs, state): seq_counts [S, 8]
    and seq_iou [S] CUMULATIVE over the stream, gt_match [R, G] of the chunk (-1 on padding rows)."""
    import numpy as np
    boxes, gt, ids, n_in, T, R, G, F, tau, _ = _score_arguments(boxes, num_objects, track_id, gt_boxes, n_frames, tau)
    S = R // F
    v_in = check_valid(valid, S, F)
    state = new_score_state(S) if state is None else {k: np.array(state[k]) for k in SCORE_STATE_KEYS}
    counts, seq_iou, gt_match = np.zeros((S, 8), np.int32), np.zeros(S, np.float64), np.full((R, G), -1, np.int32)
    for s in range(S):
        si = state["score_i"][s]
        c = dict(zip(COUNTS[:5], (int(x) for x in si[:5])))
        remembered, tracked, frames = ([int(x) for x in si[o:o + 8]] for o in (8, 16, 24))
        sum_iou = np.float64(state["score_f"][s])
        for f in range(int(v_in[s])):
            r = s * F + f
            n = int(min(max(n_in[r], 0), T))
            gt_match[r], sum_iou = _score_frame(c, remembered, tracked, frames, sum_iou, boxes[:, r], ids[:, r], n, gt[r], tau)
        si[:5], si[8:16], si[16:24], si[24:32] = [c[k] for k in COUNTS[:5]], remembered, tracked, frames
        state["score_f"][s] = sum_iou
        _score_objects(c, tracked[:G], frames[:G])
        counts[s], seq_iou[s] = [c[k] for k in COUNTS], sum_iou
    return {"seq_counts": counts, "seq_iou": seq_iou, "gt_match": gt_match}, state


def mot_summary(counts, sum_iou) -> Dict[str, float]:
    """the CLEAR-MOT figures of summed counts (COUNTS order) and the summed IoU of the matches; a denominator of 0 gives nan"""
    c = dict(zip(COUNTS, (int(v) for v in counts)))
    div = lambda a, b: a / b if b else float("nan")
    return {"mota": 1.0 - div(c["misses"] + c["fp"] + c["idsw"], c["gt"]) if c["gt"] else float("nan"),
            "motp": div(float(sum_iou), c["matches"]), "id_switches": c["idsw"],
            "mostly_tracked": div(c["mostly_tracked"], c["gt_objects"]), "mostly_lost": div(c["mostly_lost"], c["gt_objects"]),
            "false_positives": c["fp"], "misses": c["misses"], "gt": c["gt"], "matches": c["matches"], "gt_objects": c["gt_objects"]}


def reference_identity(boxes, num_objects, track_id, gt_boxes, n_frames, tau=0.5, n_ids=None):
    """air_track_idf restated in numpy float64.  boxes [T, R, 4], num_objects [R], track_id [T, R], gt_boxes [R, G, 4] (or
    [S, F, G, 4]); n_ids: None = n_frames * T.  Returns overlap [S, G, n_ids] int32 and seq_idf [S, 4] int32 (IDF_COUNTS)."""
    import numpy as np
    boxes, gt, ids, n_in, T, R, G, F, tau, n_ids = _score_arguments(boxes, num_objects, track_id, gt_boxes, n_frames, tau, n_ids)
    S = R // F
    overlap, seq_idf = np.zeros((S, G, n_ids), np.int32), np.zeros((S, 4), np.int32)
    masks = np.arange(1 << G)
    for s in range(S):
        gt_frames = hyp_frames = 0
        last_id = -1
        for f in range(F):
            r = s * F + f
            n = int(min(max(n_in[r], 0), T))
            hyp = [j for j in range(n) if ids[j, r] >= 0 and np.isfinite(boxes[j, r]).all()]
            present = [g for g in range(G) if gt[r, g, 2] > 0]
            gt_frames, hyp_frames = gt_frames + len(present), hyp_frames + len(hyp)
            for j in hyp:
                if ids[j, r] >= n_ids:
                    continue
                last_id = max(last_id, int(ids[j, r]))
                for g in present:
                    if box_iou(gt[r, g], boxes[j, r]) > tau:
                        overlap[s, g, ids[j, r]] += 1
        best = np.zeros(1 << G, np.int64)                          # best[m]: the ids so far assigned within the subset m of slots
        with_overlap = 0
        for i in range(last_id + 1):
            col = overlap[s, :, i].astype(np.int64)
            if not col.any():
                continue
            with_overlap += 1
            new = best.copy()
            for g in range(G):
                has = (masks >> g) & 1 == 1
                new[has] = np.maximum(new[has], best[masks[has] ^ (1 << g)] + col[g])
            best = new
        seq_idf[s] = [best[-1], gt_frames, hyp_frames, with_overlap]
    return {"overlap": overlap, "seq_idf": seq_idf}


def idf_summary(totals) -> Dict[str, float]:
    """the identity figures of summed seq_idf rows (IDF_COUNTS order; only the first three enter); a denominator of 0 gives nan"""
    idtp, gt_frames, hyp_frames = (int(v) for v in tuple(totals)[:3])
    div = lambda a, b: a / b if b else float("nan")
    return {"idf1": div(2 * idtp, gt_frames + hyp_frames), "idp": div(idtp, hyp_frames), "idr": div(idtp, gt_frames), "idtp": idtp,
            "idfp": hyp_frames - idtp, "idfn": gt_frames - idtp, "gt_frames": gt_frames, "hyp_frames": hyp_frames}


def _hota_score(A, sim):
    """pass 2 of HOTA: the score a pair is matched by (a function of its own so that a test can plant another rule)"""
    return A * sim


def _hota_levels(sim):
    """pass 2 of HOTA: L = the number of thresholds a match of this sim counts at: sim >= alpha_k, no epsilon"""
    return sum(1 for alpha in HOTA_ALPHAS if sim >= alpha)


def reference_hota(boxes, num_objects, track_id, gt_boxes, n_frames, n_ids=None, return_matching=False):
    """air_track_hota restated in numpy float64 and `solve_assignment`, operation for operation (HOTA in the module text).  boxes
    [T, R, 4], num_objects [R], track_id [T, R], gt_boxes [R, G, 4] (or [S, F, G, 4]); n_ids: None = n_frames * T.  Returns
    seq_hota_i [S, 19, 3] int32 (HOTA_COUNTS), seq_hota_f [S, 19, 4] float64 (HOTA_SUMS), hota_potential [S, G, n_ids] float64,
    hota_id_count [S, n_ids], hota_gt_count [S, G] and hota_matches [S, 19, G, n_ids] int32.  return_matching=True adds hota_match
    [R, G] int32: the hypothesis matched to slot g in that frame (the one matching, before any threshold), -1 for none."""
    import numpy as np
    boxes, gt, ids, n_in, T, R, G, F, _, n_ids = _score_arguments(boxes, num_objects, track_id, gt_boxes, n_frames, None, n_ids, True)
    S, NA = R // F, len(HOTA_ALPHAS)
    if S * NA * G * n_ids > 2 ** 31 - 1:
        raise ValueError("hota_matches [%d, %d, %d, %d] would have more than 2^31 - 1 elements" % (S, NA, G, n_ids))
    out = {"seq_hota_i": np.zeros((S, NA, 3), np.int32), "seq_hota_f": np.zeros((S, NA, 4), np.float64),
           "hota_potential": np.zeros((S, G, n_ids), np.float64), "hota_id_count": np.zeros((S, n_ids), np.int32),
           "hota_gt_count": np.zeros((S, G), np.int32), "hota_matches": np.zeros((S, NA, G, n_ids), np.int32)}
    hota_match = np.full((R, G), -1, np.int32)
    for s in range(S):
        pot, ic, gc, matches = out["hota_potential"][s], out["hota_id_count"][s], out["hota_gt_count"][s], out["hota_matches"][s]
        frames = []
        gt_dets = hyp_dets = 0
        for f in range(F):                                         # pass 1
            r = s * F + f
            n = int(min(max(n_in[r], 0), T))
            hyp = [j for j in range(n) if ids[j, r] >= 0 and np.isfinite(boxes[j, r]).all()]
            rows = [j for j in hyp if ids[j, r] < n_ids]           # the hypotheses that take part
            present = [g for g in range(G) if gt[r, g, 2] > 0]
            sim = np.zeros((G, T), np.float64)
            for g in present:
                for j in rows:
                    sim[g, j] = box_iou(gt[r, g], boxes[j, r])
            rs, cs = _sequential_sum(sim), _sequential_sum(sim.T)
            for g in present:
                for j in rows:
                    d = (cs[j] + rs[g]) - sim[g, j]
                    if d > HOTA_EPS:
                        pot[g, ids[j, r]] += sim[g, j] / d
                gc[g] += 1
            for j in rows:
                ic[ids[j, r]] += 1
            gt_dets, hyp_dets = gt_dets + len(present), hyp_dets + len(hyp)
            frames.append((r, rows, present, sim))
        tp, loc = np.zeros(NA, np.int64), np.zeros(NA, np.float64)
        for r, rows, present, sim in frames:                       # pass 2
            if not rows:
                continue
            profit, admissible = np.zeros((len(rows), MAX_SLOTS), np.int64), np.zeros((len(rows), MAX_SLOTS), bool)
            for q, j in enumerate(rows):
                i = ids[j, r]
                for g in present:
                    if sim[g, j] > 0.0:
                        A = pot[g, i] / ((np.float64(gc[g]) + np.float64(ic[i])) - pot[g, i])
                        profit[q, g], admissible[q, g] = 1 + int(math.floor(_hota_score(A, sim[g, j]) * PROFIT_SCALE)), True
            for q, g in enumerate(solve_assignment(profit, admissible)):
                if g >= 0:
                    hota_match[r, g] = rows[q]
            for g in range(G):                                     # the matched pairs in ascending g
                j = int(hota_match[r, g])
                if j < 0:
                    continue
                for a in range(_hota_levels(sim[g, j])):
                    tp[a] += 1
                    loc[a] = loc[a] + sim[g, j]
                    matches[a, g, ids[j, r]] += 1
        gcf, icf = gc.astype(np.float64), ic.astype(np.float64)
        for a in range(NA):                                        # the end of the sequence
            sums = [np.float64(0.0)] * 3
            for g in range(G):
                part = [np.float64(0.0)] * 3
                for i in np.nonzero(matches[a, g])[0]:             # (ascending ids)
                    c = np.float64(matches[a, g, i])
                    part[0] = part[0] + c * (c / ((gcf[g] + icf[i]) - c))
                    part[1] = part[1] + c * (c / gcf[g])
                    part[2] = part[2] + c * (c / icf[i])
                sums = [sums[k] + part[k] for k in range(3)]
            out["seq_hota_i"][s, a] = (tp[a], gt_dets - tp[a], hyp_dets - tp[a])
            out["seq_hota_f"][s, a] = (sums[0], sums[1], sums[2], loc[a])
    if return_matching:
        out["hota_match"] = hota_match
    return out


def hota_summary(totals_i, totals_f) -> Dict[str, object]:
    """The HOTA figures of summed seq_hota_i [19, 3] (HOTA_COUNTS) and seq_hota_f [19, 4] (HOTA_SUMS) rows, TrackEval's way of
    combining sequences: per threshold DetA = tp / max(1, tp + fn + fp), DetRe = tp / max(1, tp + fn), DetPr = tp / max(1, tp + fp),
    AssA / AssRe / AssPr = ass / ass_re / ass_pr over max(1, tp), LocA = loc / tp (1 when tp = 0), HOTA = sqrt(DetA AssA).  Returns
    hota, deta, assa, detre, detpr, assre, asspr, loca (the means over the 19 thresholds), hota0, loca0 (at alpha = 0.05), per_alpha
    (the 19-long lists under the same names, and alpha) and the counts gt_dets, hyp_dets; every figure nan when there was neither
    ground truth nor a hypothesis."""
    import numpy as np
    ti, tf = np.asarray(totals_i).astype(np.int64), np.asarray(totals_f, np.float64)
    NA = len(HOTA_ALPHAS)
    if ti.shape != (NA, 3) or tf.shape != (NA, 4):
        raise ValueError("hota_summary: expected totals [%d, 3] and [%d, 4], got %s and %s" % (NA, NA, ti.shape, tf.shape))
    names = ("hota", "deta", "assa", "detre", "detpr", "assre", "asspr", "loca")
    per = {k: [] for k in names}
    gt_dets, hyp_dets = int(ti[0, 0] + ti[0, 1]), int(ti[0, 0] + ti[0, 2])
    empty = gt_dets == 0 and hyp_dets == 0
    for a in range(NA):
        tp, fn, fp = (int(v) for v in ti[a])
        ass, ass_re, ass_pr, loc = (float(v) for v in tf[a])
        row = dict(deta=tp / max(1, tp + fn + fp), detre=tp / max(1, tp + fn), detpr=tp / max(1, tp + fp), assa=ass / max(1, tp),
                   assre=ass_re / max(1, tp), asspr=ass_pr / max(1, tp), loca=loc / tp if tp else 1.0)
        row["hota"] = math.sqrt(row["deta"] * row["assa"])
        for k in names:
            per[k].append(float("nan") if empty else row[k])
    out = {k: sum(per[k]) / NA for k in names}
    out.update(hota0=per["hota"][0], loca0=per["loca"][0], gt_dets=gt_dets, hyp_dets=hyp_dets)
    out["per_alpha"] = dict(per, alpha=list(HOTA_ALPHAS))
    return out


# ---- MOTS: the tracks scored as masks (the module text states the rule) ----------------------------------------------------------------------
def mots_contingency(owner, gt_instances, T, G):
    """air_score_contingency restated in numpy: owner and gt_instances [R, H, W] (or [S, F, H, W]) integer maps, -1 = background ->
    cont [R, T+1, G+1] int32, cont[r, a, b] = the pixels of image r with owner + 1 == a and gt + 1 == b.  A pixel whose owner + 1 is
    outside 0..T or whose gt + 1 is outside 0..G is counted nowhere."""
    import numpy as np
    T, G = int(T), int(G)
    if not 1 <= T <= MAX_SLOTS or not 1 <= G <= MAX_GT:
        raise ValueError("mots_contingency: T within 1..%d and G within 1..%d, got %d and %d" % (MAX_SLOTS, MAX_GT, T, G))
    o, g = np.asarray(owner), np.asarray(gt_instances)
    if o.shape != g.shape or o.ndim not in (3, 4):
        raise ValueError("mots_contingency: two maps [R, H, W] (or [S, F, H, W]) of one shape, got %s and %s" % (o.shape, g.shape))
    R = int(np.prod(o.shape[:-2]))
    a, b = o.reshape(R, -1).astype(np.int64) + 1, g.reshape(R, -1).astype(np.int64) + 1
    inside = (a >= 0) & (a <= T) & (b >= 0) & (b <= G)
    nb = (T + 1) * (G + 1)
    flat = (np.arange(R, dtype=np.int64)[:, None] * nb + a * (G + 1) + b)[inside]
    return np.bincount(flat, minlength=R * nb).astype(np.int32).reshape(R, T + 1, G + 1)


def _mots_gt_area(counts, g):
    """col[g]: the area of ground-truth slot g, over EVERY owner row -- the background's and those of steps that are no hypothesis
    included (a function of its own so that a test can plant another rule)"""
    return sum(int(v) for v in counts[:, g + 1])


def _mots_is_match(inter, union):
    """mask IoU > 1/2, strictly, in integers (a function of its own so that a test can plant another rule)"""
    return inter > union - inter


def reference_mots(cont, num_objects, track_id, n_frames):
    """air_track_mots restated in Python integers and numpy float64, with the kernel's bits (MOTS in the module text).  cont
    [R, T+1, G+1] (mots_contingency's, or air_score_contingency's), num_objects [R], track_id [T, R], R = S * n_frames.  Returns
    seq_mots_i [S, 8] int32 (MOTS_COUNTS), seq_mots_f [S] float64, mots_match [R, G] int32, mots_iou [R, G] float32."""
    import numpy as np
    cont = np.asarray(cont)
    if cont.ndim != 3 or not np.issubdtype(cont.dtype, np.integer):
        raise ValueError("reference_mots: cont must be an integer table [R, T+1, G+1], got %s %s" % (cont.shape, cont.dtype))
    R, T, G, F = int(cont.shape[0]), int(cont.shape[1]) - 1, int(cont.shape[2]) - 1, int(n_frames)
    if not 1 <= T <= MAX_SLOTS:
        raise ValueError("reference_mots: 1..%d objects per frame, got %d" % (MAX_SLOTS, T))
    if not 1 <= G <= MAX_GT:
        raise ValueError("reference_mots: 1..%d ground-truth slots, got %d" % (MAX_GT, G))
    if F < 1 or R < 1 or R % F:
        raise ValueError("reference_mots: %d rows are not sequences of %d frames" % (R, F))
    if R * (T + 1) * (G + 1) > 2 ** 31 - 1:
        raise ValueError("reference_mots: cont [%d, %d, %d] would have more than 2^31 - 1 elements" % (R, T + 1, G + 1))
    ids, n_in = np.asarray(track_id).astype(np.int64), np.asarray(num_objects).astype(np.int64).reshape(-1)
    if ids.shape != (T, R) or n_in.shape != (R,):
        raise ValueError("reference_mots: expected track_id [%d, %d] and num_objects [%d], got %s and %s"
                         % (T, R, R, ids.shape, n_in.shape))
    S = R // F
    out = {"seq_mots_i": np.zeros((S, 8), np.int32), "seq_mots_f": np.zeros(S, np.float64),
           "mots_match": np.full((R, G), -1, np.int32), "mots_iou": np.zeros((R, G), np.float32)}
    for s in range(S):
        remembered, tracked, present = [-1] * G, [0] * G, [0] * G
        c = dict.fromkeys(MOTS_COUNTS, 0)
        soft = np.float64(0.0)
        for f in range(F):
            r = s * F + f
            counts = cont[r]
            n = int(min(max(n_in[r], 0), T))
            row = [sum(int(v) for v in counts[j + 1]) for j in range(T)]
            col = [_mots_gt_area(counts, g) for g in range(G)]
            hyp = [j for j in range(n) if ids[j, r] >= 0 and row[j] > 0]
            taken = set()
            for g in range(G):
                if not col[g] > 0:
                    continue
                c["gt"] += 1
                present[g] += 1
                pairs = [(j, int(counts[j + 1, g + 1])) for j in hyp]
                pairs = [(j, inter) for j, inter in pairs if _mots_is_match(inter, row[j] + col[g] - inter)]
                if not pairs:
                    c["fn"] += 1
                    continue
                j, inter = pairs[0]                                # (at most one on a non-negative table)
                taken.add(j)
                with np.errstate(all="ignore"):
                    iou = np.float64(inter) / np.float64(row[j] + col[g] - inter)
                c["tp"] += 1
                tracked[g] += 1
                soft = soft + iou
                c["ids"] += 1 if remembered[g] >= 0 and remembered[g] != ids[j, r] else 0
                remembered[g] = int(ids[j, r])
                out["mots_match"][r, g], out["mots_iou"][r, g] = j, np.float32(iou)
            c["fp"] += len(set(hyp) - taken)
        _score_objects(c, tracked, present)
        out["seq_mots_i"][s] = [c[k] for k in MOTS_COUNTS]
        out["seq_mots_f"][s] = soft
    return out


def mots_summary(totals_i, soft) -> Dict[str, float]:
    """the MOTS figures of summed seq_mots_i rows (MOTS_COUNTS order) and the summed seq_mots_f: motsa = (tp - fp - ids) / gt, smotsa =
    (soft - fp - ids) / gt, motsp = soft / tp, recall = tp / gt, precision = tp / (tp + fp), mostly_tracked and mostly_lost (fractions
    of the ground-truth objects), and the counts; a denominator of 0 gives nan"""
    c = dict(zip(MOTS_COUNTS, (int(v) for v in totals_i)))
    if len(c) != len(MOTS_COUNTS):
        raise ValueError("mots_summary: expected the %d counters %s" % (len(MOTS_COUNTS), ", ".join(MOTS_COUNTS)))
    soft = float(soft)
    div = lambda a, b: a / b if b else float("nan")
    return {"motsa": div(c["tp"] - c["fp"] - c["ids"], c["gt"]), "smotsa": div(soft - c["fp"] - c["ids"], c["gt"]),
            "motsp": div(soft, c["tp"]), "recall": div(c["tp"], c["gt"]), "precision": div(c["tp"], c["tp"] + c["fp"]),
            "mostly_tracked": div(c["mostly_tracked"], c["gt_objects"]), "mostly_lost": div(c["mostly_lost"], c["gt_objects"]),
            "id_switches": c["ids"], "false_positives": c["fp"], "misses": c["fn"], "gt": c["gt"], "tp": c["tp"],
            "gt_objects": c["gt_objects"], "soft": soft}


# ---- STITCHING: track fragments joined across long occlusions (the module text states the rule) -------------------------------------------
STITCH_MAX_GAP = 8                 # max_gap's default (provisional)
STITCHED, STITCH_OVERFLOW = 0, 1   # stitch_status
STITCH_PER_TRACK = ("stitch_parent", "stitch_root", "stitch_d2", "stitch_affinity")                # [S, 32]
STITCH_TABLES = ("stitch_first", "stitch_last", "stitch_length", "stitch_gaps")                    # [S, F T]
STITCH_OUTPUTS = ("stitch_id",) + STITCH_PER_TRACK + STITCH_TABLES + ("num_links", "stitch_status")
STITCH_ON_A_STREAM = ("stitching is out of scope on a stream: it is a second pass over the WHOLE tracks of a sequence, and a stream has "
                      "only the chunk and the live table; track the sequence in one call and bind TrackStitcher to that SequenceTracker")
STITCH_WITH_SMOOTH = ("stitch= together with smooth= is not supported: the smoother's completed table assumes that a track spanning a "
                      "frame was seen within max_age frames of it (trajectory.completed_rows), which a stitched track is not")


def check_stitch(max_gap=STITCH_MAX_GAP, gate=True, appearance_weight=DEFAULTS["appearance_weight"], noise=None):
    """Refuse what air_track_stitch refuses of its rule arguments (pure host code).  noise: None (trajectory.DEFAULTS) or a dict with
    any of process_noise, measurement_noise, velocity_var, held to the smoother's supported domain by `check_motion`.  Returns
    (max_gap, gate, w, the complete noise dict)."""
    if isinstance(max_gap, bool) or not isinstance(max_gap, int) and int(max_gap) != max_gap or int(max_gap) < 1:
        raise ValueError("max_gap must be an integer >= 1, got %r" % (max_gap,))
    if int(max_gap) > 2 ** 31 - 1:
        raise ValueError("max_gap must fit int32, got %r" % (max_gap,))
    if gate is None or gate is False:
        raise ValueError("stitching needs a gate: True (MOTION_GATE_DEFAULT) or a finite squared Mahalanobis distance > 0, got %r" % (gate,))
    gate = check_motion_gate(gate, True)
    w = float(appearance_weight)
    if not (math.isfinite(w) and 0.0 <= w <= 1.0):
        raise ValueError("appearance_weight must be a number within [0, 1], got %r" % (appearance_weight,))
    return int(max_gap), gate, w, check_motion(noise or True)


def _stitch_ends(sightings_a, sightings_b):
    """the pair's step: the sighting (frame, slot) of a whose `what` row enters the msd and from whose frame the gap is counted -- its
    LAST --, and that of b whose `where` and `what` rows are compared -- its FIRST (a function of its own so that a test can plant
    another rule)"""
    return sightings_a[-1], sightings_b[0]


def _stitch_gaps(gaps, links):
    """relabel: the gaps of a root -- the chain's own and one per link"""
    return gaps + links


def reference_stitch(what, where, track_id, num_tracks, track_first, track_last, track_length, track_gaps, n_frames,
                     max_gap=STITCH_MAX_GAP, gate=True, appearance_weight=DEFAULTS["appearance_weight"], process_noise=None,
                     measurement_noise=None, velocity_var=None, return_state=False, return_margins=False):
    """air_track_stitch restated in numpy float64 and `solve_assignment` (STITCHING in the module text).  what [T, R, A], where
    [T, R, 4] fp32, track_id [T, R], num_tracks [S], track_first / _last / _length / _gaps [S, F T], R = S * n_frames.  Returns
    STITCH_OUTPUTS: stitch_id [T, R] int32, stitch_parent, stitch_root [S, 32] int32, stitch_d2, stitch_affinity [S, 32] float32,
    stitch_first, stitch_last, stitch_length, stitch_gaps [S, F T] int32, num_links, stitch_status [S] int32.  return_state=True adds
    stitch_state: (s, id) -> the filtered state (x, v, Pxx, Pxv, Pvv) of the track's own filter at its last sighting, and
    stitch_pairs: (s, a, b) -> (d2, msd, aff | None for an inadmissible pair) of every candidate pair, in float64;
    return_margins=True adds gate_margin [S]: the smallest |d2 - gate| over the candidate pairs (inf without one)."""
    import numpy as np
    from .trajectory import _filter_start
    terms = {k: v for k, v in dict(process_noise=process_noise, measurement_noise=measurement_noise, velocity_var=velocity_var).items()
             if v is not None}
    max_gap, gate, w, terms = check_stitch(max_gap, gate, appearance_weight, terms)
    what, where = np.asarray(what, np.float32), np.asarray(where, np.float32)
    ids = np.asarray(track_id).astype(np.int32)
    T, R, A = what.shape
    T, F, S = check_arguments(T, n_frames, R)
    FT = F * T
    if where.shape != (T, R, 4) or ids.shape != (T, R):
        raise ValueError("where / track_id: expected %s and %s, got %s and %s" % ((T, R, 4), (T, R), where.shape, ids.shape))
    tables = [np.asarray(t).astype(np.int32) for t in (track_first, track_last, track_length, track_gaps)]
    num_tracks = np.asarray(num_tracks).astype(np.int64)
    if num_tracks.shape != (S,) or any(t.shape != (S, FT) for t in tables):
        raise ValueError("num_tracks [%d] and the four track tables [%d, %d] expected" % (S, S, FT))
    (q_shift, q_scale), r, vv = terms["process_noise"], terms["measurement_noise"], terms["velocity_var"]
    q = np.array([q_scale, q_shift, q_scale, q_shift], np.float64)
    out = {"stitch_id": ids.copy(), "stitch_parent": np.full((S, MAX_SLOTS), -1, np.int32),
           "stitch_root": np.full((S, MAX_SLOTS), -1, np.int32), "stitch_d2": np.zeros((S, MAX_SLOTS), np.float32),
           "stitch_affinity": np.zeros((S, MAX_SLOTS), np.float32), "num_links": np.zeros(S, np.int32),
           "stitch_status": np.zeros(S, np.int32)}
    out.update({k: t.copy() for k, t in zip(STITCH_TABLES, tables)})
    states, pairs, gate_margin = {}, {}, np.full(S, np.inf)
    clip =lambda f: min(max(int(f), 0), F - 1)
    for s in range(S):
        N = max(int(num_tracks[s]), 0)
        if N > MAX_SLOTS:                                          # OVERFLOW: the sequence passes through
            out["stitch_status"][s] = STITCH_OVERFLOW
            out["stitch_root"][s] = np.arange(MAX_SLOTS)
            continue
        N = min(N, FT)                                             # (no more ids than objects: the table rows end at F T)
        first, last, length, gaps = (t[s] for t in tables)
        sightings, filt = {}, {}
        for i in range(N):                                         # filter: the track's own, over its sightings in frame order
            seen, state, prev = [], None, None
            for f in range(clip(first[i]), clip(last[i]) + 1):
                hit = np.flatnonzero(ids[:, s * F + f] == i)
                if not hit.size:
                    continue
                j = int(hit[0])
                z = where[j, s * F + f].astype(np.float64)
                with np.errstate(all="ignore"):
                    state = _filter_start(z, r, vv) if state is None else _motion_advance(state, f - prev, z, q, r)
                seen.append((f, j))
                prev = f
            if seen:
                sightings[i], filt[i] = seen, state
                states[(s, i)] = state
        profit, admissible = np.zeros((N, MAX_SLOTS), np.int64), np.zeros((N, MAX_SLOTS), bool)
        d2s, affs = {}, {}
        for a in sightings:                                        # pair
            for b in sightings:
                (fa, ja), (fb, jb) = _stitch_ends(sightings[a], sightings[b])
                g = fb - fa
                if not 1 <= g <= max_gap:
                    continue
                with np.errstate(all="ignore"):
                    xp, s_in = _motion_predicted_state(filt[a], g, q, r)
                    d2 = float(_motion_d2(xp, s_in, where[jb, s * F + fb].astype(np.float64)))
                    d = what[ja, s * F + fa].astype(np.float64) - what[jb, s * F + fb].astype(np.float64)
                    msd = float(_sequential_sum(d * d) / np.float64(A))
                    gate_margin[s] = min(gate_margin[s], abs(d2 - gate))
                    v = _gated_pair(d2, msd, w, gate, None, None)
                if v is not None and not v >= 0.0:
                    v = None
                pairs[(s, a, b)] = (d2, msd, v)
                if v is None:
                    continue
                profit[b, a], admissible[b, a] = 1 + int(math.floor(v * PROFIT_SCALE)), True
                d2s[(a, b)], affs[(a, b)] = d2, v
        parent, child = out["stitch_parent"][s], {}
        for b, a in enumerate(solve_assignment(profit, admissible)):       # links
            if a >= 0:
                parent[b], child[int(a)] = a, b
                out["stitch_d2"][s, b], out["stitch_affinity"][s, b] = np.float32(d2s[(int(a), b)]), np.float32(affs[(int(a), b)])
        out["num_links"][s] = len(child)
        for i in range(N):                                         # relabel
            root = i
            while parent[root] >= 0:
                root = int(parent[root])
            out["stitch_root"][s, i] = root
            if parent[i] >= 0:
                for k, empty in zip(STITCH_TABLES, (-1, -1, 0, 0)):
                    out[k][s, i] = empty
                continue
            tail, total, total_gaps, links = i, int(length[i]), int(gaps[i]), 0
            while tail in child:
                tail, links = child[tail], links + 1
                total, total_gaps = total + int(length[tail]), total_gaps + int(gaps[tail])
            out["stitch_last"][s, i], out["stitch_length"][s, i] = last[tail], total
            out["stitch_gaps"][s, i] = _stitch_gaps(total_gaps, links)
        cols = ids[:, s * F:(s + 1) * F]
        inside = (cols >= 0) & (cols < N)
        out["stitch_id"][:, s * F:(s + 1) * F] = np.where(inside, out["stitch_root"][s][np.where(inside, cols, 0)], cols)
    if return_state:
        out["stitch_state"], out["stitch_pairs"] = states, pairs
    if return_margins:
        out["gate_margin"] = gate_margin
    return out


# ---- the launch arguments by name ------------------------------------------------------------------------------------------------------
# The parameters of every air_track_* entry this module launches, in the order of include/air_hip.h and without the trailing stream
# (tests/test_track_optimal_host.py holds each tuple to the header's prototype).  A plan entry is the values filed under these names.
_ROWS, _SHAPE = ("what", "boxes", "score", "num_objects"), ("T", "S", "F", "R", "A")
_RULE = ("iou_gate", "appearance_weight", "birth_score", "max_age")
_PER_OBJECT = ("track_id", "obj_state", "affinity", "prev_frame", "prev_slot")
_TABLES = ("num_tracks", "track_first", "track_last", "track_length", "track_gaps", "state_counts")
_MOTION = (("what", "where", "boxes", "score", "num_objects") + _SHAPE + ("H", "W") + _RULE
           + ("matching", "q_shift", "q_scale", "measurement_noise", "velocity_var"))
_SCORED, _SCORE_SHAPE = ("boxes", "num_objects", "track_id", "gt_boxes"), ("T", "G", "S", "F", "R")
MOT_OUTPUTS = ("seq_counts", "seq_iou", "gt_match")
ENTRY_ARGS = {
    "air_track_associate": _ROWS + _SHAPE + _RULE + _PER_OBJECT + _TABLES,
    "air_track_associate_motion": _MOTION + _PER_OBJECT + _TABLES + ("pred_where", "pred_boxes"),
    "air_track_associate_motion_gated": _MOTION + ("gate_d2",) + _PER_OBJECT + _TABLES + ("pred_where", "pred_boxes", "pred_d2"),
    "air_track_associate_stream": (_ROWS + _SHAPE + _RULE + ("valid", "matching", "st_seq", "st_slots", "st_box", "st_what") + _PER_OBJECT
                                   + ("state_counts", "num_retired") + RETIRED),
    "air_track_owner": ("owner", "track_id", "T", "R", "H", "W", "track_owner"),
    "air_track_score": _SCORED + ("tau",) + _SCORE_SHAPE + MOT_OUTPUTS,
    "air_track_score_stream": _SCORED + ("tau",) + _SCORE_SHAPE + ("valid", "st_i", "st_f") + MOT_OUTPUTS,
    "air_track_idf": _SCORED + ("tau",) + _SCORE_SHAPE + ("n_ids", "overlap", "seq_idf"),
    "air_track_hota": _SCORED + _SCORE_SHAPE + ("n_ids", "potential", "id_count", "gt_count", "matches", "seq_hota_i", "seq_hota_f"),
}
ENTRY_ARGS["air_track_associate_optimal"] = ENTRY_ARGS["air_track_associate"]


# air_track_mots' parameters in the same way.  It is no key of ENTRY_ARGS: that table is held to the ten entries above by
# tests/test_track_optimal_host.py, as air_track_stitch's tuple (STITCH_ARGS) stands beside it for the same reason.
MOTS_ARGS = ("cont", "num_objects", "track_id") + _SCORE_SHAPE + MOTS_OUTPUTS


def plan_entry(L, name, values):
    """the plan entry of air_track_* `name`: values[n] of every parameter n of its prototype, in the prototype's order"""
    return (getattr(L, name), tuple(values[n] for n in ENTRY_ARGS[name]), name)


class IdentityScores:
    """The identity metric of a stage (the tracker on its own table, the smoother on its two): the air_track_score launch of every
    key used so far with its buffers and graph (`entries`, at most four: a sweep over tau must not pile up buffers and graphs), the
    staging copy of the ground truth, and the running totals on the device.  An entry made with identity=True runs air_track_idf
    behind air_track_score (one graph still) and feeds `totals_idf`.  HOTA has a cache of its own (`hota_entries`, at most two, keyed
    by (table, G): the air_track_hota launch, its buffers and graph) and totals of its own (`totals_hota_i`, `totals_hota_f`).  So
    has MOTS (`mots_entries`, at most two, keyed by (table, G): the unchanged air_score_contingency and air_track_mots as one plan and
    one graph, the int8 staging copy of the instance maps, cont and the four outputs; `totals_mots_i`, `totals_mots_f`); a MOTS table
    is (T rows, frames per sequence, owner map, counts, ids).  A stage on a STREAM holds one entry, air_track_score_stream's
    (`stream_entry`), and keeps no totals: its counts are cumulative.  A TABLE is what a launch scores: (T rows, frames per
    sequence, boxes, counts, ids)."""

    def __init__(self, stage, S):
        import torch
        self.stage, self.engine, self.S, self.entries = stage, stage.engine, int(S), {}
        dev = self.engine.device
        with torch.cuda.device(dev):
            self.totals_i = torch.zeros((8,), dtype=torch.int64, device=dev)
            self.totals_f = torch.zeros((1,), dtype=torch.float64, device=dev)
            self.totals_idf = torch.zeros((4,), dtype=torch.int64, device=dev)
            self.totals_hota_i = torch.zeros((len(HOTA_ALPHAS), 3), dtype=torch.int64, device=dev)
            self.totals_hota_f = torch.zeros((len(HOTA_ALPHAS), 4), dtype=torch.float64, device=dev)
            self.totals_mots_i = torch.zeros((8,), dtype=torch.int64, device=dev)
            self.totals_mots_f = torch.zeros((1,), dtype=torch.float64, device=dev)
        self.hota_entries = {}                                     # (table, G) -> buffers, plan, graph: at most two, apart from `entries`
        self.mots_entries = {}                                     # (table, G) -> buffers, plan, graph: at most two, apart from both

    # ---- the cache ------------------------------------------------------------------------------------------------------------------
    def _cached(self, cache, limit, key, build):
        """the entry of `cache` under `key`; a miss is what build() makes, captured when the stage holds a graph, and the oldest entries
        are evicted, their graphs destroyed, while there would be more than `limit`"""
        entry = cache.get(key)
        if entry is None:
            entry = build()
            if self.stage._graph is not None:
                self.engine.synchronize()
                entry["graph"] = self.engine._capture_plans([entry["plan"]])
            while len(cache) >= limit:
                destroy_graphs([cache.pop(next(iter(cache)))["graph"]])
            cache[key] = entry
        return entry

    @staticmethod
    def _check(G, tau=None, n_ids=None):
        """the refusals of an entry's arguments, in the one order every entry has them (None: the entry does not take it)"""
        if n_ids is not None and not 1 <= int(n_ids) <= MAX_IDS:
            raise ValueError("n_ids must be within 1..%d, got %r" % (MAX_IDS, n_ids))
        if not 1 <= G <= MAX_GT:
            raise ValueError("gt_boxes: 1..%d ground-truth slots, got %d" % (MAX_GT, G))
        if tau is not None and not 0.0 <= float(tau) <= 1.0:
            raise ValueError("tau must be within [0, 1], got %r" % (tau,))

    def _zeros(self, **buffers):
        """an entry without plan and graph yet: a zeroed device buffer of every name=(shape, dtype)"""
        import torch
        dev = self.engine.device
        with torch.cuda.device(dev):
            return dict({k: torch.zeros(shape, dtype=dtype, device=dev) for k, (shape, dtype) in buffers.items()}, graph=None)

    def _mot_buffers(self, N, G):
        """the four CLEAR-MOT buffers of a table of N columns: gt_boxes, seq_counts, seq_iou, gt_match"""
        import torch
        return self._zeros(gt_boxes=((N, G, 4), torch.float32), seq_counts=((self.S, 8), torch.int32),
                           seq_iou=((self.S,), torch.float64), gt_match=((N, G), torch.int32))

    def _launch(self, name, table, entry, **more):
        """the plan entry `name` on `table`: the buffers of `entry` filed under their own names, `more` under the prototype's"""
        T, n_frames, boxes, counts, ids = table
        L, p = self.stage._H.lib(), self.stage._H._p
        values = {k: p(v) for k, v in entry.items() if k not in ("plan", "graph")}
        values.update(boxes=p(boxes), num_objects=p(counts), track_id=p(ids), T=T, G=int(entry["gt_boxes"].shape[1]), S=self.S,
                      F=n_frames, R=self.S * n_frames, **more)
        return plan_entry(L, name, values)

    def entry(self, key, G, tau, table, identity=False, n_ids=None):
        """the air_track_score launch on `table` with its buffers -- gt_boxes, seq_counts, seq_iou, gt_match -- kept under key +
        (G, tau); captured when the stage holds a graph.  identity=True: kept under key + (G, tau, "idf"), with air_track_idf behind
        it and its buffers seq_idf, idf_overlap [S, G, n_ids]"""
        import torch
        G, tau_f = int(G), float(tau)

        def build():
            self._check(G, tau, n_ids if identity else None)
            entry = self._mot_buffers(self.S * table[1], G)
            entry["plan"] = [self._launch("air_track_score", table, entry, tau=tau_f)]
            if identity:
                entry.update(self._zeros(seq_idf=((self.S, 4), torch.int32), idf_overlap=((self.S, G, int(n_ids)), torch.int32)))
                entry["plan"].append(self._launch("air_track_idf", table, entry, tau=tau_f, n_ids=int(n_ids),
                                                  overlap=self.stage._H._p(entry["idf_overlap"])))
            return entry
        return self._cached(self.entries, 4, key + (G, tau_f) + (("idf",) if identity else ()), build)

    def stream_entry(self, G, tau, table, valid, state, clash, invalid=None):
        """the ONE entry of a stream, under (G, tau): air_track_score_stream on `table` with the valid-count buffer `valid` and the
        score state carried between the chunks (state["score_i"], state["score_f"]), its buffers those of `entry`.  Another key is
        refused with the stage's own text `clash` % (the key held, the key asked for); `invalid` % (MAX_GT, G, tau), where the stage
        has one text for a G or a tau out of range"""
        key = (int(G), float(tau))

        def build():
            if self.entries:
                raise ValueError(clash % (next(iter(self.entries)), key))
            if invalid is not None and not (1 <= key[0] <= MAX_GT and 0.0 <= key[1] <= 1.0):
                raise ValueError(invalid % (MAX_GT, key[0], tau))
            self._check(key[0], tau)
            p = self.stage._H._p
            entry = self._mot_buffers(self.S * table[1], key[0])
            entry["plan"] = [self._launch("air_track_score_stream", table, entry, tau=key[1], valid=p(valid), st_i=p(state["score_i"]),
                                          st_f=p(state["score_f"]))]
            return entry
        return self._cached(self.entries, 1, key, build)

    def run(self, gt_boxes, n_frames, entry_for):
        """stage gt_boxes [N, G, 4] or [S, n_frames, G, 4] into the buffers of `entry_for(G)` and issue that entry; returns it"""
        import torch
        eng, N = self.engine, self.S * n_frames
        gb = torch.as_tensor(gt_boxes)
        if gb.dim() not in (3, 4) or gb.shape[-1] != 4 or gb.numel() != N * gb.shape[-2] * 4:
            raise ValueError("gt_boxes: expected [%d, G, 4] or [%d, %d, G, 4], got %s" % (N, self.S, n_frames, tuple(gb.shape)))
        entry = entry_for(gb.shape[-2])
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            entry["gt_boxes"].copy_(gb.reshape(entry["gt_boxes"].shape), non_blocking=True)
        if gb.is_cuda:
            gb.record_stream(eng.stream)
        eng._replay_or_run(entry["graph"], entry["plan"])
        return entry

    def _accumulate(self, accumulate, entry, **totals):
        """every total=source: the sum of entry[source] over the sequences is added to the running total of that name (accumulate) or
        restarts it (not), on the device with no read-back; returns the totals by name"""
        import torch
        with torch.cuda.stream(self.engine.stream):
            for name, source in totals.items():
                total = getattr(self, name)
                part = entry[source].sum(0, dtype=total.dtype).reshape(total.shape)
                if accumulate:
                    total += part
                else:
                    total.copy_(part)
        return {name: getattr(self, name) for name in totals}

    def result(self, entry, accumulate=None):
        """the entry's outputs; accumulate True / False: added to / restarting the totals on the device (no read-back), and the totals"""
        identity = {"totals_idf": "seq_idf"} if "seq_idf" in entry else {}
        out = {k: entry[k] for k in MOT_OUTPUTS + (("seq_idf", "idf_overlap") if identity else ())}
        if accumulate is not None:
            out.update(self._accumulate(accumulate, entry, totals_i="seq_counts", totals_f="seq_iou", **identity))
        self.engine.wait_for_engine()
        return out

    def run_stream(self, gt_boxes, tau, table, *stream_entry_args):
        """stage gt_boxes, issue the stream's entry (`stream_entry`'s arguments behind the table) and return its outputs: seq_counts
        and seq_iou cumulative over the stream, gt_match of the chunk"""
        return self.result(self.run(gt_boxes, table[1], lambda G: self.stream_entry(G, tau, table, *stream_entry_args)))

    def stream_summary(self) -> Dict[str, float]:
        """mot_summary of a stream so far: the cumulative seq_counts and seq_iou of its entry summed over the S sequences at read-back
        (ONE read-back; no totals are kept on the device).  Nothing scored yet: the figures of nothing (nan rates)."""
        import torch
        self.engine.wait_for_engine()
        if not self.entries:
            return mot_summary([0] * 8, 0.0)
        entry = next(iter(self.entries.values()))
        flat = torch.cat([entry["seq_counts"].sum(0, dtype=torch.int64).double(), entry["seq_iou"].sum(0, keepdim=True)]).tolist()
        return mot_summary(flat[:8], flat[8])

    def hota_entry(self, key, G, table, n_ids):
        """the air_track_hota launch on `table` with its buffers -- gt_boxes, seq_hota_i, seq_hota_f, hota_potential, hota_id_count,
        hota_gt_count, hota_matches -- kept in `hota_entries` under key + (G,); captured (one graph) when the stage holds a graph.
        `entries` and its keys are not touched."""
        import torch
        S, N, NA = self.S, self.S * table[1], len(HOTA_ALPHAS)
        G, n_ids = int(G), int(n_ids)

        def build():
            self._check(G, n_ids=n_ids)
            if S * NA * G * n_ids > 2 ** 31 - 1:
                raise ValueError("hota_matches [%d, %d, %d, %d] would have more than 2^31 - 1 elements" % (S, NA, G, n_ids))
            i32, f64, p = torch.int32, torch.float64, self.stage._H._p
            entry = self._zeros(gt_boxes=((N, G, 4), torch.float32), seq_hota_i=((S, NA, 3), i32), seq_hota_f=((S, NA, 4), f64),
                                hota_potential=((S, G, n_ids), f64), hota_id_count=((S, n_ids), i32), hota_gt_count=((S, G), i32),
                                hota_matches=((S, NA, G, n_ids), i32))
            entry["plan"] = [self._launch("air_track_hota", table, entry, n_ids=n_ids, potential=p(entry["hota_potential"]),
                                          id_count=p(entry["hota_id_count"]), gt_count=p(entry["hota_gt_count"]),
                                          matches=p(entry["hota_matches"]))]
            return entry
        return self._cached(self.hota_entries, 2, key + (G,), build)

    def run_hota(self, gt_boxes, n_frames, entry_for, accumulate=None):
        """stage gt_boxes into the buffers of `entry_for(G)` (a hota_entry), issue it and return its outputs; accumulate True / False:
        added to / restarting totals_hota_i [19, 3] int64 and totals_hota_f [19, 4] float64 on the device (no read-back), and they"""
        entry = self.run(gt_boxes, n_frames, entry_for)
        out = {k: entry[k] for k in ("seq_hota_i", "seq_hota_f", "hota_potential", "hota_id_count", "hota_gt_count", "hota_matches")}
        if accumulate is not None:
            out.update(self._accumulate(accumulate, entry, totals_hota_i="seq_hota_i", totals_hota_f="seq_hota_f"))
        self.engine.wait_for_engine()
        return out

    def mots_entry(self, key, G, table):
        """the MOTS plan on `table` = (T rows, frames per sequence, owner map [N, H, W] int8, counts, ids): the unchanged
        air_score_contingency of (owner map, the staged instance maps), then air_track_mots, with their buffers -- gt_instances
        [N, H, W] int8, cont [N, T+1, G+1], seq_mots_i, seq_mots_f, mots_match, mots_iou -- kept in `mots_entries` under key + (G,);
        captured (ONE graph of both launches) when the stage holds a graph.  `entries`, `hota_entries` and their keys are not touched."""
        import torch
        T, n_frames, owner, counts, ids = table
        S, N, G = self.S, self.S * n_frames, int(G)

        def build():
            if not 1 <= G <= MAX_GT:
                raise ValueError("mots: 1..%d ground-truth slots, got %d" % (MAX_GT, G))
            if owner.dtype != torch.int8 or owner.dim() != 3 or owner.shape[0] != N:
                raise ValueError("mots: the owner map must be int8 [%d, H, W], got %s %s" % (N, owner.dtype, tuple(owner.shape)))
            Hi, Wi = (int(v) for v in owner.shape[1:])
            i32, L, p = torch.int32, self.stage._H.lib(), self.stage._H._p
            entry = self._zeros(gt_instances=((N, Hi, Wi), torch.int8), cont=((N, T + 1, G + 1), i32), seq_mots_i=((S, 8), i32),
                                seq_mots_f=((S,), torch.float64), mots_match=((N, G), i32), mots_iou=((N, G), torch.float32))
            values = {k: p(v) for k, v in entry.items() if k != "graph"}
            values.update(num_objects=p(counts), track_id=p(ids), T=T, G=G, S=S, F=n_frames, R=N)
            entry["plan"] = [(L.air_score_contingency, (p(owner), values["gt_instances"], T, G, N, Hi, Wi, values["cont"]),
                              "air_score_contingency"),
                             (L.air_track_mots, tuple(values[k] for k in MOTS_ARGS), "air_track_mots")]
            return entry
        return self._cached(self.mots_entries, 2, key + (G,), build)

    def run_mots(self, gt_instances, key, G, table, accumulate=None):
        """stage gt_instances [N, H, W] or [S, n_frames, H, W] (integers, -1 = background; a label from G on is counted nowhere) into
        the buffers of `mots_entry(key, G, table)`, issue it and return its outputs and cont; accumulate True / False: added to /
        restarting totals_mots_i [8] int64 and totals_mots_f [1] float64 on the device (no read-back), and they"""
        import torch
        eng, shape = self.engine, (self.S * table[1],) + tuple(int(v) for v in table[2].shape[1:])
        gi = torch.as_tensor(gt_instances)
        if gi.dim() not in (3, 4) or tuple(gi.shape[-2:]) != shape[1:] or gi.numel() != shape[0] * shape[1] * shape[2]:
            raise ValueError("gt_instances: expected [%d, %d, %d] or [%d, %d, %d, %d], got %s"
                             % (shape + (self.S, table[1]) + shape[1:] + (tuple(gi.shape),)))
        entry = self.mots_entry(key, G, table)
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            entry["gt_instances"].copy_(gi.reshape(shape), non_blocking=True)
        if gi.is_cuda:
            gi.record_stream(eng.stream)
        eng._replay_or_run(entry["graph"], entry["plan"])
        out = {k: entry[k] for k in MOTS_OUTPUTS + ("cont",)}
        if accumulate is not None:
            out.update(self._accumulate(accumulate, entry, totals_mots_i="seq_mots_i", totals_mots_f="seq_mots_f"))
        eng.wait_for_engine()
        return out

    def score_entries(self):
        """every {"plan", "graph"} entry of the three caches: what a stage captures and releases with its own graph"""
        return list(self.entries.values()) + list(self.hota_entries.values()) + list(self.mots_entries.values())

    def reset(self):
        """zero the totals"""
        import torch
        eng = self.engine
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            self.totals_i.zero_()
            self.totals_f.zero_()
            self.totals_idf.zero_()
            self.totals_hota_i.zero_()
            self.totals_hota_f.zero_()
            self.totals_mots_i.zero_()
            self.totals_mots_f.zero_()
        eng.wait_for_engine()

    def summary(self) -> Dict[str, float]:
        """mot_summary of everything accumulated since the last reset (ONE read-back)"""
        import torch
        self.engine.wait_for_engine()
        flat = torch.cat([self.totals_i.double(), self.totals_f]).tolist()
        return mot_summary(flat[:8], flat[8])

    def identity_summary(self) -> Dict[str, float]:
        """idf_summary of everything scored with identity=True since the last reset (ONE read-back)"""
        self.engine.wait_for_engine()
        return idf_summary(self.totals_idf.tolist())

    def hota_summary(self) -> Dict[str, object]:
        """hota_summary of everything `hota` took since the last reset (ONE read-back)"""
        import torch
        self.engine.wait_for_engine()
        NA = len(HOTA_ALPHAS)
        flat = torch.cat([self.totals_hota_i.double().reshape(-1), self.totals_hota_f.reshape(-1)]).tolist()
        return hota_summary([[int(v) for v in flat[3 * a:3 * a + 3]] for a in range(NA)],
                            [flat[3 * NA + 4 * a:3 * NA + 4 * a + 4] for a in range(NA)])


    def mots_summary(self) -> Dict[str, float]:
        """mots_summary of everything `mots` took since the last reset (ONE read-back)"""
        import torch
        self.engine.wait_for_engine()
        flat = torch.cat([self.totals_mots_i.double(), self.totals_mots_f]).tolist()
        return mots_summary(flat[:8], flat[8])


class TrackerBase(BoundStage):
    """What SequenceTracker and StreamTracker share: the binding and its refusals, the association rule, the per-object outputs with
    state_counts and track_owner, the launch list (the association entry, then air_track_owner), the provider's call with its checks
    and an IdentityScores.  A subclass allocates what is its own behind this constructor and then `_rebuild()`s; it states its
    association entry (`_associate`), the provider rows it reads next to `what` (`_read_rows`) and its own part of `result`."""
    ACCEPTS = ("scene", "refiner", "subset", "tiled")
    REFUSALS = TiledSceneParser.REFUSALS

    def __init__(self, provider, n_frames, iou_gate, appearance_weight, birth_score, max_age, matching):
        self._rows = self.bind(provider)
        T, F, S = check_arguments(provider.T, n_frames, provider.R, iou_gate, appearance_weight, birth_score, max_age, matching)
        import torch
        from . import hip as H
        self.provider, self.engine = provider, provider.engine
        self._bound = provider
        self.T, self.R, self.S, self.F = T, int(provider.R), S, F
        self.iou_gate, self.appearance_weight, self.birth_score, self.max_age = (float(iou_gate), float(appearance_weight),
                                                                                 float(birth_score), int(max_age))
        self.matching = matching
        self._what = self._rows["what"]
        self.A = int(self._what.shape[-1])
        self.img_size = tuple(int(v) for v in provider.owner.shape[1:])
        R, z = self.R, self._zeros
        self.track_id, self.obj_state, self.affinity = z((T, R)), z((T, R), torch.int8), z((T, R), torch.float32)
        self.prev_frame, self.prev_slot = z((T, R)), z((T, R))
        self.state_counts = z((S, 6))
        self.track_owner = z((R,) + self.img_size, torch.int16)
        self._H = H
        self.scores = IdentityScores(self, S)
        self._score = self.scores.entries                          # (G, tau) -> buffers, plan, graph

    def _zeros(self, shape, dtype=None):
        import torch
        dev = self.engine.device
        with torch.cuda.device(dev):
            return torch.zeros(shape, dtype=torch.int32 if dtype is None else dtype, device=dev)

    def _build_plan(self):
        """nothing of the engine's configuration is held by the tracker's launch list: built once"""
        provider, (Hi, Wi) = self.provider, self.img_size
        L, p = self._H.lib(), self._H._p
        values = dict(what=p(self._what), boxes=p(provider.boxes), score=p(provider.score), num_objects=p(provider.num_objects),
                      T=self.T, S=self.S, F=self.F, R=self.R, A=self.A, H=Hi, W=Wi, iou_gate=self.iou_gate,
                      appearance_weight=self.appearance_weight, birth_score=self.birth_score, max_age=self.max_age,
                      matching=MATCHINGS.index(self.matching), state_counts=p(self.state_counts), owner=p(provider.owner),
                      track_owner=p(self.track_owner), **{k: p(getattr(self, k)) for k in _PER_OBJECT})
        associate, own = self._associate(p)
        values.update(own)
        self.segments = OrderedDict([("associate", [plan_entry(L, associate, values)]),
                                     ("owner", [plan_entry(L, "air_track_owner", values)])])
        self._plan = [e for seg in self.segments.values() for e in seg]

    def _associate(self, p):
        """(the association entry's name, its values next to the shared ones): the subclass's"""
        raise NotImplementedError

    def _read_rows(self):
        """the keys of the provider's rows() that the association reads next to `what` (`run_provider` holds the provider to them)"""
        return ()

    def _score_entries(self):
        return self.scores.score_entries()

    def _score_table(self):
        """the table the metrics score: the provider's boxes and counts with this tracker's ids"""
        return (self.T, self.F, self.provider.boxes, self.provider.num_objects, self.track_id)

    def check_frames(self, frames):
        """frames as a tensor of [S, F, H, W]"""
        import torch
        frames = torch.as_tensor(frames)
        Hi, Wi = self.img_size
        if frames.numel() != self.R * Hi * Wi or frames.dim() < 2 or tuple(frames.shape[:2]) != (self.S, self.F):
            raise ValueError("expected frames [%d, %d, %d, %d], got %s" % (self.S, self.F, Hi, Wi, tuple(frames.shape)))
        return frames

    def run_provider(self, frames, *args, **kwargs):
        """the bound provider's `parse()` on the frames as its R = S F rows (further arguments go to it unchanged)"""
        par = self.provider
        base = par.parse(self.check_frames(frames).reshape(self.R, *self.img_size), *args, **kwargs)
        expected = dict(what=self._what, boxes=par.boxes, score=par.score, num_objects=par.num_objects, owner=par.owner)
        expected.update({k: self._rows[k] for k in self._read_rows()})
        self.check_same_buffers(base, expected, "tracker", bound="provider")
        return base

    def result(self, base=None):
        out = dict(base) if base is not None else {}
        out.update({k: getattr(self, k) for k in _PER_OBJECT}, state_counts=self.state_counts, track_owner=self.track_owner)
        return out


class SequenceTracker(TrackerBase):
    def __init__(self, provider, n_frames, iou_gate=DEFAULTS["iou_gate"], appearance_weight=DEFAULTS["appearance_weight"],
                 birth_score=DEFAULTS["birth_score"], max_age=DEFAULTS["max_age"], matching="greedy", motion=None, motion_gate=None):
        """motion: None (every track is matched against its last-sighting box), True (against its predicted box, MOTION in the module
        text, with trajectory.DEFAULTS) or a dict with any of process_noise=(q_shift, q_scale), measurement_noise, velocity_var --
        what `smooth=` and `fit_track_noise` use.  motion_gate (needs motion): None (the pairs are gated by the IoU with the
        predicted box), True (MOTION_GATE_DEFAULT, provisional) or a squared Mahalanobis distance > 0: THE GATE in the module text"""
        super().__init__(provider, n_frames, iou_gate, appearance_weight, birth_score, max_age, matching)
        self.motion = check_motion(motion)
        self.motion_gate = check_motion_gate(motion_gate, self.motion)
        import torch
        T, R, S, FT, z = self.T, self.R, self.S, self.F * self.T, self._zeros
        self.num_tracks = z((S,))
        self.track_first, self.track_last, self.track_length, self.track_gaps = z((S, FT)), z((S, FT)), z((S, FT)), z((S, FT))
        if self.motion is not None:
            self.pred_where, self.pred_boxes = z((T, R, 4), torch.float32), z((T, R, 4), torch.float32)
        if self.motion_gate is not None:
            self.pred_d2 = z((T, R), torch.float32)
        self.totals_i, self.totals_f, self.totals_idf = self.scores.totals_i, self.scores.totals_f, self.scores.totals_idf
        self._rebuild()
        self.engine.synchronize()

    def _associate(self, p):
        """greedy and optimal have an entry each; motion has the one entry of both matchings, the gate another: still one launch"""
        own, m = {k: p(getattr(self, k)) for k in _TABLES[:-1]}, self.motion
        if m is None:
            return "air_track_associate_optimal" if self.matching == "optimal" else "air_track_associate", own
        own.update(where=p(self._rows["where"]), q_shift=m["process_noise"][0], q_scale=m["process_noise"][1],
                   measurement_noise=m["measurement_noise"], velocity_var=m["velocity_var"], pred_where=p(self.pred_where),
                   pred_boxes=p(self.pred_boxes))
        if self.motion_gate is None:
            return "air_track_associate_motion", own
        own.update(gate_d2=self.motion_gate, pred_d2=p(self.pred_d2))
        return "air_track_associate_motion_gated", own

    def _read_rows(self):
        return ("where",) if self.motion is not None else ()               # the rows the filter reads

    def launch_count(self) -> Dict[str, int]:
        """entries of one `track()` call behind the bound provider's own (`parser` holds that provider's launch_count())"""
        return {"parser": self.provider.launch_count(), "track_associate": 1, "track_owner": 1}

    # ---- tracking -----------------------------------------------------------------------------------------------------------
    def track(self, frames, *args, **kwargs):
        """frames [S, F, H, W]; further arguments go to the provider's `parse()` unchanged (its rows are the frames, row s F + f).
        Returns the provider's dict of device tensors, untouched, and next to it (the NEXT call overwrites them): track_id [T, R] int32
        (-1 = none), obj_state [T, R] int8 (STATES), affinity [T, R] (aff of the match, 0 unless matched), prev_frame, prev_slot [T, R]
        int32 (the track's previous sighting, -1 unless matched), num_tracks [S] int32, track_first, track_last, track_length,
        track_gaps [S, F * T] int32 per id (-1 / -1 / 0 / 0 from num_tracks[s] on), state_counts [S, 6] int32, track_owner
        [R, H, W] int16 (the track id a pixel belongs to, -1 = background or an object without a track); with motion also pred_where,
        pred_boxes [T, R, 4] (for a MATCHED object the prediction of its track that the match was made against, else 0); with
        motion_gate also pred_d2 [T, R] (the squared Mahalanobis distance of the matched pair, else 0).  Same stream contract as
        SceneParser.parse: the work runs on the engine's stream, on return the caller's current stream is ordered after it, and the
        next call waits for the caller's reads before it overwrites them."""
        eng = self.engine
        base = self.run_provider(frames, *args, **kwargs)
        eng._replay_or_run(self._graph, self._plan)
        eng.wait_for_engine()
        return self.result(base)

    def result(self, base=None):
        out = super().result(base)
        out.update({k: getattr(self, k) for k in _TABLES[:-1]})
        if self.motion is not None:
            out.update(pred_where=self.pred_where, pred_boxes=self.pred_boxes)
        if self.motion_gate is not None:
            out.update(pred_d2=self.pred_d2)
        return out

    # ---- the identity metric ------------------------------------------------------------------------------------------------
    def _score_entry(self, G, tau, identity=False):
        return self.scores.entry((), G, tau, self._score_table(), identity, self.F * self.T)

    def score(self, gt_boxes, tau=0.5, accumulate=True, identity=False):
        """Score the LATEST `track()` against gt_boxes [R, G, 4] (or [S, F, G, 4]; G <= 8; slot g is the same object in every frame of
        a sequence, width <= 0 = absent).  Returns device tensors that the next call with the same (G, tau) overwrites: seq_counts
        [S, 8] int32 (COUNTS), seq_iou [S] float64, gt_match [R, G] int32, and the running totals_i [8] int64 / totals_f [1] float64,
        which this call adds to (accumulate=False: restarts) on the device, with no read-back.  identity=True runs air_track_idf
        behind air_track_score and adds seq_idf [S, 4] int32 (IDF_COUNTS), idf_overlap [S, G, F * T] int32 and the running totals_idf
        [4] int64 (`identity_summary()` reads them).  Same stream contract as `track`."""
        return self.scores.result(self.scores.run(gt_boxes, self.F, lambda G: self._score_entry(G, tau, bool(identity))),
                                  bool(accumulate))

    def hota(self, gt_boxes, accumulate=True):
        """HOTA of the LATEST `track()` against gt_boxes as `score` takes them (air_track_hota; HOTA in the module text; n_ids = F T).
        Returns device tensors that the next call with the same G overwrites: seq_hota_i [S, 19, 3] int32 (HOTA_COUNTS), seq_hota_f
        [S, 19, 4] float64 (HOTA_SUMS), hota_potential [S, G, F T] float64, hota_id_count [S, F T], hota_gt_count [S, G],
        hota_matches [S, 19, G, F T] int32, and the running totals_hota_i [19, 3] int64 / totals_hota_f [19, 4] float64, which this
        call adds to (accumulate=False: restarts) on the device, with no read-back.  `score` and its cache are not touched.  Same
        stream contract as `track`."""
        return self.scores.run_hota(gt_boxes, self.F, lambda G: self.scores.hota_entry((), G, self._score_table(), self.F * self.T),
                                    bool(accumulate))

    def hota_summary(self) -> Dict[str, object]:
        """The HOTA figures of everything `hota` took since the last reset (ONE read-back): hota, deta, assa, detre, detpr, assre,
        asspr, loca (means over the 19 thresholds), hota0, loca0 (at alpha = 0.05), per_alpha; nan with nothing to score."""
        return self.scores.hota_summary()

    def _mots_table(self):
        """the table MOTS scores: the provider's step owner map and counts with this stage's ids"""
        return (self.T, self.F, self.provider.owner, self.provider.num_objects, self._score_table()[4])

    def mots(self, gt_instances, n_slots=MAX_GT, accumulate=True):
        """MOTS of the LATEST `track()` against gt_instances [R, H, W] (or [S, F, H, W]; integers, -1 = background; label g is the same
        object in every frame of a sequence, a label from n_slots on is counted nowhere): the unchanged air_score_contingency of the
        provider's owner map and the instance maps, then air_track_mots (MOTS in the module text; 1 <= n_slots <= 8).  Returns device
        tensors that the next call with the same n_slots overwrites: seq_mots_i [S, 8] int32 (MOTS_COUNTS), seq_mots_f [S] float64,
        mots_match [R, n_slots] int32, mots_iou [R, n_slots] fp32, cont [R, T+1, n_slots+1] int32, and the running totals_mots_i [8]
        int64 / totals_mots_f [1] float64, which this call adds to (accumulate=False: restarts) on the device, with no read-back.
        `score`, `hota` and their caches are not touched.  Same stream contract as `track`."""
        return self.scores.run_mots(gt_instances, (), n_slots, self._mots_table(), bool(accumulate))

    def mots_summary(self) -> Dict[str, float]:
        """The MOTS figures of everything `mots` took since the last reset (ONE read-back): motsa, smotsa, motsp, recall, precision,
        mostly_tracked, mostly_lost and the counts; nan with nothing to score."""
        return self.scores.mots_summary()

    def reset(self):
        """zero the totals"""
        self.scores.reset()

    def summary(self) -> Dict[str, float]:
        """The figures of everything scored since the last reset (ONE read-back): mota = 1 - (misses + fp + idsw) / gt, motp =
        sum_iou / matches, id_switches, mostly_tracked, mostly_lost (fractions of the ground-truth objects), false_positives, misses,
        and the counts gt, matches, gt_objects.  A denominator of 0 gives nan."""
        return self.scores.summary()

    def identity_summary(self) -> Dict[str, float]:
        """The identity figures of everything scored with identity=True since the last reset (ONE read-back): idf1 = 2 idtp /
        (gt_frames + hyp_frames), idp = idtp / hyp_frames, idr = idtp / gt_frames, and the counts idtp, idfp, idfn, gt_frames,
        hyp_frames.  A denominator of 0 gives nan."""
        return self.scores.identity_summary()


class StreamTracker(TrackerBase):
    """Identities over a STREAM: S sequences of any length fed in chunks of `chunk_frames` frames, the track table, the id counter and
    the last sightings (box and a bit copy of the `what` row) carried on the device between the calls (include/air_hip.h states the
    layout; nothing is read back between chunks).  Chunk invariance: whatever the chunking -- ragged `valid`, valid = 0 included -- a
    sequence gets the ids, states, previous sightings and affinity bits SequenceTracker would give on the concatenation of its valid
    frames, with prev_frame and the tracks' first / last as GLOBAL frame indices.  Binds to the providers SequenceTracker binds to (a
    temporal.TemporalProposer sees only its chunk) and refuses the same ones with the same wording.  One `push` is the provider's
    `parse()` and then ONE hipGraph after `capture()`: air_track_associate_stream, air_track_owner.

    A push MUTATES the state, captured or not: pushing a chunk twice continues the stream with a repeated chunk, it does not repeat the
    call -- `state_dict()` before and `load_state_dict()` after is how a chunk is re-run.  Ids: 0..32766 per sequence until `reset`;
    a birth beyond is OVERFLOW.  Out of scope on a stream: IDF1 and HOTA (their tables are indexed by global id), MOTS (there is no
    `mots`: the carried score state has a fixed layout, st_i [S, 32] and st_f [S], with no room for a second metric's map, per-slot
    counts and sum), more than 32 live tracks.  Trajectories: a trajectory.StreamSmoother bound to this tracker (fixed-lag
    smoothing, `lag` frames late; the forecast at once)."""

    def __init__(self, provider, chunk_frames, iou_gate=DEFAULTS["iou_gate"], appearance_weight=DEFAULTS["appearance_weight"],
                 birth_score=DEFAULTS["birth_score"], max_age=DEFAULTS["max_age"], matching="greedy", motion=None, motion_gate=None):
        if (motion is not None and motion is not False) or (motion_gate is not None and motion_gate is not False):
            raise ValueError(MOTION_ON_A_STREAM)
        super().__init__(provider, chunk_frames, iou_gate, appearance_weight, birth_score, max_age, matching)
        import numpy as np
        import torch
        S, z = self.S, self._zeros
        self.num_retired = z((S,))
        self.retired = {k: z((S, MAX_SLOTS + self.F * self.T)) for k in RETIRED}
        self.valid = z((S,))
        self.state = {"seq": z((S, 2)), "slots": z((S, 8, MAX_SLOTS)), "box": z((S, MAX_SLOTS, 4), torch.float32),
                      "what": z((S, MAX_SLOTS, self.A), torch.float32), "score_i": z((S, 32)), "score_f": z((S,), torch.float64)}
        self.frames_seen = np.zeros(S, np.int64)                   # the host's mirror of state["seq"][:, 0]
        # `valid` is staged in pinned memory and copied without blocking the host; a ring, so that the host waits only for the copy
        # of four pushes ago (long done) before it reuses a buffer, never for the chunk that is still running
        self._valid_ring = [(torch.zeros((S,), dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(4)]
        self._pushes = 0
        self._rebuild()
        self.reset()
        self.engine.synchronize()

    def _associate(self, p):
        st = self.state
        return "air_track_associate_stream", dict(valid=p(self.valid), st_seq=p(st["seq"]), st_slots=p(st["slots"]), st_box=p(st["box"]),
                                                  st_what=p(st["what"]), num_retired=p(self.num_retired),
                                                  **{k: p(self.retired[k]) for k in RETIRED})

    def launch_count(self) -> Dict[str, int]:
        """entries of one `push()` behind the bound provider's own (`parser` holds that provider's launch_count())"""
        return {"parser": self.provider.launch_count(), "track_associate_stream": 1, "track_owner": 1}

    # ---- the state ------------------------------------------------------------------------------------------------------------
    def reset(self, sequences=None):
        """Restart all (None) or some sequences ON THE DEVICE -- a slot reused for a new video: frames_seen and next_id 0, no live
        track, and the sequence's score state with them (read `summary()` first if its figures matter).  No read-back."""
        import numpy as np
        import torch
        rows = np.arange(self.S) if sequences is None else np.atleast_1d(np.asarray(sequences, np.int64))
        if rows.size and (rows.min() < 0 or rows.max() >= self.S):
            raise ValueError("reset: sequences within 0..%d, got %r" % (self.S - 1, sequences))
        eng, st = self.engine, self.state
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            idx = torch.as_tensor(rows, device=eng.device)
            empty = torch.tensor(ST_EMPTY, dtype=torch.int32, device=eng.device)
            st["seq"][idx] = 0
            st["slots"][idx] = empty[None, :, None].expand(len(rows), 8, MAX_SLOTS)
            st["box"][idx] = 0
            st["what"][idx] = 0
            st["score_i"][idx] = 0
            st["score_i"][idx, 8:16] = -1
            st["score_f"][idx] = 0
        self.frames_seen[rows] = 0
        eng.wait_for_engine()

    def score_reset(self):
        """restart the identity metric of every sequence (the association state stays)"""
        import torch
        eng, st = self.engine, self.state
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            st["score_i"].zero_()
            st["score_i"][:, 8:16] = -1
            st["score_f"].zero_()
            for e in self._score.values():
                e["seq_counts"].zero_()
                e["seq_iou"].zero_()
        eng.wait_for_engine()

    def live(self):
        """the live tracks as VIEWS of the state (device tensors the next push rewrites): live, id, age, length, gaps, first,
        last_frame, last_slot [S, 32] int32 (ST_FIELDS; a slot with live == 0 holds ST_EMPTY), box [S, 32, 4], what [S, 32, A]"""
        out = {k: self.state["slots"][:, i] for i, k in enumerate(ST_FIELDS)}
        out.update(box=self.state["box"], what=self.state["what"])
        return out

    def state_dict(self):
        """a copy of the carried state as plain device tensors (STATE_KEYS + SCORE_STATE_KEYS): checkpoint, or re-run a chunk"""
        import torch
        eng = self.engine
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            out = {k: v.clone() for k, v in self.state.items()}
        eng.wait_for_engine()
        return out

    def load_state_dict(self, state):
        """take a state `state_dict()` gave (any device; score keys optional): copied INTO the buffers the graph holds; frames_seen is
        read back once for the host's mirror"""
        import torch
        eng = self.engine
        for k in STATE_KEYS:
            if tuple(state[k].shape) != tuple(self.state[k].shape):
                raise ValueError("load_state_dict: %s has shape %s, this stream's is %s"
                                 % (k, tuple(state[k].shape), tuple(self.state[k].shape)))
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            for k, buf in self.state.items():
                if k in state:
                    buf.copy_(torch.as_tensor(state[k]).to(buf.dtype), non_blocking=True)
        eng.wait_for_engine()
        eng.synchronize()
        self.frames_seen[:] = self.state["seq"][:, 0].cpu().numpy()

    # ---- tracking -----------------------------------------------------------------------------------------------------------
    def push(self, frames, valid=None, *args, **kwargs):
        """The next chunk: frames [S, F, H, W], valid [S] integers on the host (None: every frame; sequence s has its first
        clip(valid[s], 0, F) frames in this chunk, the rest of its rows is padding whose contents do not matter -- the provider still
        parses them); further arguments go to the provider's `parse()` unchanged.  Returns the provider's dict of device tensors,
        untouched, and next to it (the NEXT push overwrites them): track_id, obj_state, affinity, prev_frame (GLOBAL frame index),
        prev_slot [T, R] (-1 / ABSENT / 0 / -1 / -1 on padding rows), state_counts [S, 6] (valid frames), num_retired [S] and retired_id
        / _first / _last / _length / _gaps [S, 32 + F * T] (the tracks retired in this chunk; the live ones: `live()`), track_owner
        [R, H, W] int16.  A chunk that would take frames_seen past int32 is refused before anything runs.  The push mutates the state:
        not idempotent (the class text).  Same stream contract as SequenceTracker.track: the work runs on the engine's stream, on
        return the caller's current stream is ordered after it, and the next call waits for the caller's reads before it overwrites
        them."""
        import numpy as np
        import torch
        eng = self.engine
        if torch.is_tensor(valid):
            valid = valid.cpu().numpy()
        v = check_valid(valid, self.S, self.F)
        after = check_frames_seen(self.frames_seen, v)
        frames = self.check_frames(frames)
        # `valid` goes to the device ahead of the parse, on the engine's stream: behind the launches that read the buffer for the
        # chunk before (its tail, its score), in front of this chunk's tail; the host runs on
        staged, copied = self._valid_ring[self._pushes % len(self._valid_ring)]
        self._pushes += 1
        copied.synchronize()
        staged.copy_(torch.from_numpy(v.astype(np.int32)))
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            self.valid.copy_(staged, non_blocking=True)
            copied.record(eng.stream)
        base = self.run_provider(frames, *args, **kwargs)
        eng._replay_or_run(self._graph, self._plan)
        self.frames_seen = after
        eng.wait_for_engine()
        return self.result(base)

    def result(self, base=None):
        out = super().result(base)
        out.update(num_retired=self.num_retired, **self.retired)
        return out

    # ---- the identity metric ------------------------------------------------------------------------------------------------
    def score(self, gt_boxes, tau=0.5):
        """Score the LATEST chunk against gt_boxes [R, G, 4] (or [S, F, G, 4]; G <= 8; slot g is the same object over the whole stream
        of a sequence, width <= 0 = absent; padding rows are not read), continuing the stream's metric: an identity switch at a chunk
        boundary counts.  Once per push -- like the push it mutates its state.  Returns device tensors the next call overwrites:
        seq_counts [S, 8] int32 (COUNTS) and seq_iou [S] float64 CUMULATIVE over the stream, gt_match [R, G] int32 of the chunk."""
        return self.scores.run_stream(gt_boxes, tau, self._score_table(), self.valid, self.state,
                                      "this stream is scored with (G, tau) = %r; call score_reset() with nothing pushed in between, or a "
                                      "stream of its own, for %r")

    def summary(self) -> Dict[str, float]:
        """mot_summary of the stream so far: the cumulative seq_counts and seq_iou summed over the S sequences at read-back (ONE
        read-back; no totals are kept on the device).  Nothing scored yet: the figures of nothing (nan rates)."""
        return self.scores.stream_summary()


# ---- stitching behind a tracker ------------------------------------------------------------------------------------------------------------
# air_track_stitch's parameters in the order of include/air_hip.h, without the trailing stream (ENTRY_ARGS holds the entries the trackers
# themselves launch)
STITCH_ARGS = (("what", "where", "track_id", "num_tracks", "track_first", "track_last", "track_length", "track_gaps", "T", "S", "F", "R",
                "A", "max_gap", "gate_d2", "appearance_weight", "q_shift", "q_scale", "measurement_noise", "velocity_var")
               + STITCH_OUTPUTS)


class TrackStitcher(BoundStage):
    """Track fragments joined across occlusions longer than max_age (STITCHING in the module text), behind a SequenceTracker -- with or
    without motion=, under either matching; a StreamTracker is refused (STITCH_ON_A_STREAM).  Binds to the tracker (what parameters and
    switches are forwarded to) and only READS it and its provider: ONE hipGraph of two launches behind the tracker's own --
    air_track_stitch on the tracker's ids and tables and the provider's what / where rows, then the unchanged air_track_owner on
    stitch_id into a `track_owner` buffer of this stage.  appearance_weight=None: the tracker's; noise=None: the tracker's motion
    terms if it has them, else trajectory.DEFAULTS; max_gap and gate (True: MOTION_GATE_DEFAULT) are provisional.  It owns an
    IdentityScores over (T, F, the provider's boxes and counts, stitch_id): score / hota / mots / summary / identity_summary /
    hota_summary / mots_summary / reset are SequenceTracker's, on the stitched ids (n_ids stays F T: the ids are not compacted; MOTS
    reads the provider's owner map with stitch_id)."""

    def __init__(self, tracker, max_gap=STITCH_MAX_GAP, gate=True, appearance_weight=None, noise=None):
        if isinstance(tracker, StreamTracker):
            raise ValueError(STITCH_ON_A_STREAM)
        if not isinstance(tracker, SequenceTracker):
            raise ValueError("TrackStitcher binds to a track.SequenceTracker, got %s" % type(tracker).__name__)
        self.max_gap, self.gate, self.appearance_weight, self.noise = check_stitch(
            max_gap, gate, tracker.appearance_weight if appearance_weight is None else appearance_weight,
            tracker.motion if noise is None else noise)
        import torch
        from . import hip as H
        self.tracker, self.provider, self.engine = tracker, tracker.provider, tracker.engine
        self._bound = tracker
        self.T, self.R, self.S, self.F, self.A, self.img_size = tracker.T, tracker.R, tracker.S, tracker.F, tracker.A, tuple(tracker.img_size)
        self._rows = {k: tracker._rows[k] for k in ("what", "where")}
        self._H = H
        dev, S, FT = self.engine.device, self.S, self.F * self.T
        z = lambda shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.stitch_id = z((self.T, self.R))
            self.stitch_parent, self.stitch_root = z((S, MAX_SLOTS)), z((S, MAX_SLOTS))
            self.stitch_d2, self.stitch_affinity = z((S, MAX_SLOTS), torch.float32), z((S, MAX_SLOTS), torch.float32)
            self.stitch_first, self.stitch_last, self.stitch_length, self.stitch_gaps = z((S, FT)), z((S, FT)), z((S, FT)), z((S, FT))
            self.num_links, self.stitch_status = z((S,)), z((S,))
            self.track_owner = z((self.R,) + self.img_size, torch.int16)
        self.scores = IdentityScores(self, S)
        self._score = self.scores.entries
        self.totals_i, self.totals_f, self.totals_idf = self.scores.totals_i, self.scores.totals_f, self.scores.totals_idf
        self._rebuild()
        self.engine.synchronize()

    def _build_plan(self):
        """nothing of the engine's configuration is held by the launch list: built once"""
        tk, par, (Hi, Wi) = self.tracker, self.provider, self.img_size
        L, p, m = self._H.lib(), self._H._p, self.noise
        values = dict(what=p(self._rows["what"]), where=p(self._rows["where"]), T=self.T, S=self.S, F=self.F, R=self.R, A=self.A,
                      max_gap=self.max_gap, gate_d2=self.gate, appearance_weight=self.appearance_weight, q_shift=m["process_noise"][0],
                      q_scale=m["process_noise"][1], measurement_noise=m["measurement_noise"], velocity_var=m["velocity_var"],
                      **{k: p(getattr(tk, k)) for k in ("track_id",) + _TABLES[:-1]}, **{k: p(getattr(self, k)) for k in STITCH_OUTPUTS})
        owner = dict(owner=p(par.owner), track_id=p(self.stitch_id), T=self.T, R=self.R, H=Hi, W=Wi, track_owner=p(self.track_owner))
        self.segments = OrderedDict([("stitch", [(L.air_track_stitch, tuple(values[n] for n in STITCH_ARGS), "air_track_stitch")]),
                                     ("owner", [plan_entry(L, "air_track_owner", owner)])])
        self._plan = [e for seg in self.segments.values() for e in seg]

    def _score_entries(self):
        return self.scores.score_entries()

    def _score_table(self):
        """the table the metrics score: the provider's boxes and counts with the STITCHED ids"""
        return (self.T, self.F, self.provider.boxes, self.provider.num_objects, self.stitch_id)

    def launch_count(self) -> Dict[str, object]:
        """entries of one `run()` behind the tracker's own (`tracker` holds that tracker's launch_count())"""
        return {"tracker": self.tracker.launch_count(), "track_stitch": 1, "track_owner": 1}

    # ---- stitching ------------------------------------------------------------------------------------------------------------------
    def run(self, base=None):
        """stitch the tracker's LATEST `track()`; `base` (that call's result) is passed through into the returned dict and, when
        given, held to the buffers the launch list was built on.  The tracker's and the provider's buffers are only read.  Same
        stream contract as SequenceTracker.track."""
        eng = self.engine
        if base is not None:
            self.check_same_buffers(base, dict(what=self._rows["what"], where=self._rows["where"], track_id=self.tracker.track_id,
                                               num_tracks=self.tracker.num_tracks), "stitcher", bound="tracker")
        eng.wait_for_caller()
        eng._replay_or_run(self._graph, self._plan)
        eng.wait_for_engine()
        return self.result(base)

    def stitch(self, frames, *args, **kwargs):
        """the bound tracker's `track(frames, ...)`, then `run()` on its result"""
        return self.run(self.tracker.track(frames, *args, **kwargs))

    track = stitch                                                 # (the name the model's `track` calls on the last stage of a stack)

    def result(self, base=None):
        """Device tensors that the NEXT call overwrites, next to `base` (the tracker's dict, untouched -- its track_id and track_owner
        stay the tracker's): STITCH_OUTPUTS -- stitch_id [T, R] int32, stitch_parent, stitch_root [S, 32] int32, stitch_d2,
        stitch_affinity [S, 32] fp32, stitch_first / _last / _length / _gaps [S, F T] int32, num_links, stitch_status [S] int32 -- and
        stitch_owner [R, H, W] int16: air_track_owner of stitch_id (this stage's `track_owner`)."""
        out = dict(base) if base is not None else {}
        out.update({k: getattr(self, k) for k in STITCH_OUTPUTS}, stitch_owner=self.track_owner)
        return out

    # ---- the identity metrics: SequenceTracker's methods as they are, on this stage's table -------------------------------------------------
    _score_entry, score, hota = SequenceTracker._score_entry, SequenceTracker.score, SequenceTracker.hota
    summary, identity_summary, hota_summary = SequenceTracker.summary, SequenceTracker.identity_summary, SequenceTracker.hota_summary
    _mots_table, mots, mots_summary = SequenceTracker._mots_table, SequenceTracker.mots, SequenceTracker.mots_summary
    reset = SequenceTracker.reset
