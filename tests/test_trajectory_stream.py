"""GPU tests of the stream smoother's kernels (csrc/trajectory_kernels.hip: air_track_stash, air_track_smooth_stream,
air_track_smooth_tail, air_track_fill_stream) pushed chunk by chunk against trajectory.reference_smooth_stream, and device against
device against the one-shot air_track_smooth.

Bars.  EVERY output element and the carried state after every chunk are compared exactly, by bytes: the rule is float64 with only
+ - * / in one stated order, contraction off on the device.  The inputs are finite, so no NaN is made."""
import numpy as np
import pytest
import torch

from test_trajectory import ORDER, TABLE_DTYPES, check_tables, dev_t, run_smooth, sentinel, table_shapes
from test_trajectory_stream_host import planted
from track_stream_cases import chunkings, same
from trajectory_stream_cases import IMG, NOISE, cut, push, stream_case

from attend_infer_repeat_amd import trajectory
from attend_infer_repeat_amd.trajectory import ABSENT, FILLED, OBSERVED

pytestmark = pytest.mark.gpu

ROWS = ("what", "glimpse", "score")


class DeviceStream:
    """the carried state and the row ring on the device, a sentinel tail behind each; `push` is air_track_stash,
    air_track_smooth_stream and air_track_fill_stream on both tables, every output sentinel-filled before the launch"""

    def __init__(self, S, F, T, A, G, lag, max_age, horizon=0, noise=NOISE):
        from attend_infer_repeat_amd import hip as Hh
        self.Hh, self.L, self.p = Hh, Hh.lib(), Hh._p
        self.S, self.F, self.T, self.A, self.G, self.lag, self.max_age, self.Hz = S, F, T, A, G, lag, max_age, horizon
        self.C, self.D = trajectory.completed_rows(T, max_age), trajectory.ring_depth(F, lag, max_age)
        self.noise = dict(trajectory.DEFAULTS, **(noise or {}))
        fresh = trajectory.new_smooth_state(S, F, lag, max_age, T, A, G)
        packed = trajectory.pack_smooth_state(fresh)
        self.state_bytes = int(self.L.air_track_smooth_stream_state_bytes(S, self.D))
        assert self.state_bytes == packed.size
        self.state_fill = 0xA5
        self.state = torch.full((packed.size + 64,), self.state_fill, dtype=torch.uint8, device="cuda")
        self.state[:packed.size] = torch.from_numpy(packed).cuda()
        self.rings = {}
        for k in ROWS:
            flat, view, fill = sentinel(fresh[k].shape, torch.float32)
            view[:fresh[k].size] = 0
            self.rings[k] = (flat, view, fill, fresh[k].shape)

    def state_host(self):
        """(the packed state's bytes, {key: row ring}, whether the tails behind them are untouched)"""
        clean = bool((self.state[self.state_bytes:] == self.state_fill).all())
        rings = {}
        for k, (flat, view, fill, shp) in self.rings.items():
            n = int(np.prod(shp))
            rings[k] = view[:n].view(shp).cpu().numpy()
            clean = clean and bool((view[n:] == fill).all())
        return self.state[:self.state_bytes].cpu().numpy(), rings, clean

    def check_state(self, ref_state):
        packed, rings, clean = self.state_host()
        assert clean
        want = trajectory.unpack_smooth_state(trajectory.pack_smooth_state(ref_state), self.S, self.D)
        for k, v in trajectory.unpack_smooth_state(packed, self.S, self.D).items():
            assert same(v, want[k]), ("state", k, np.argwhere(v != want[k])[:4])
        for k in ROWS:
            assert same(rings[k], ref_state[k]), ("ring", k)

    def _fill(self, bufs, pre, N, per_seq):
        p = self.p
        outs = {k: sentinel(shp, torch.float32) + (shp,) for k, shp in (("what", (self.C, N, self.A)), ("glimpse", (self.C, N, self.G)),
                                                                         ("score", (self.C, N)))}
        st = self.L.air_track_fill_stream(p(self.rings["what"][1]), p(self.rings["glimpse"][1]), p(self.rings["score"][1]),
                                          p(bufs[pre + "state"][1]), p(bufs[pre + "src_frame"][1]), p(bufs[pre + "src_slot"][1]), self.T,
                                          self.S, self.D, self.C, N, per_seq, self.A, self.G, p(outs["what"][1]), p(outs["glimpse"][1]),
                                          p(outs["score"][1]), self.Hh._stream())
        assert st == 0
        return {pre + k: v for k, v in outs.items()}

    def push(self, c, stash=True, fill=True, **kw):
        """one chunk (trajectory_stream_cases.cut); returns status, {name: host array}, whether every tail is untouched, the fills"""
        L, p, S, F, T, Hz, C = self.L, self.p, self.S, self.F, self.T, self.Hz, self.C
        R, N = S * F, S * Hz
        d = {k: dev_t(c[k]) for k in ("where", "what", "glimpse", "score", "track_id")}
        d["n"], d["valid"] = dev_t(c["n"].astype(np.int32)), dev_t(np.asarray(c["valid"]).astype(np.int32))
        bufs = {}
        for pre, cols in (("sm_", R), ("fc_", N)):
            if cols:
                bufs.update({pre + k: sentinel(shp, TABLE_DTYPES[k]) + (shp,) for k, shp in table_shapes(C, cols).items()})
        for k, shp in (("sm_counts", (S, 3)), ("emit_frame", (S, F)), ("num_emitted", (S,))):
            bufs[k] = sentinel(shp, torch.int32) + (shp,)
        a = dict(where=p(d["where"]), n=p(d["n"]), track_id=p(d["track_id"]), valid=p(d["valid"]), T=T, S=S, F=F, R=R, C=C, L=self.lag,
                 Hz=Hz, D=self.D, max_age=self.max_age, H=IMG[0], W=IMG[1], q_shift=self.noise["process_noise"][0],
                 q_scale=self.noise["process_noise"][1], r=self.noise["measurement_noise"], velocity_var=self.noise["velocity_var"],
                 state=p(self.state), state_bytes=self.state_bytes)
        a.update({k: p(v[1]) for k, v in bufs.items()})
        for k in ORDER:
            a.setdefault("fc_" + k, None)
        a.update(kw)
        if stash and not kw:
            st = L.air_track_stash(p(d["what"]), p(d["glimpse"]), p(d["score"]), a["valid"], a["state"], T, S, F, R, self.A, self.G,
                                   self.D, p(self.rings["what"][1]), p(self.rings["glimpse"][1]), p(self.rings["score"][1]),
                                   self.Hh._stream())
            assert st == 0
        st = L.air_track_smooth_stream(a["where"], a["n"], a["track_id"], a["valid"], a["T"], a["S"], a["F"], a["R"], a["C"], a["L"],
                                       a["Hz"], a["D"], a["max_age"], a["H"], a["W"], float(a["q_shift"]), float(a["q_scale"]),
                                       float(a["r"]), float(a["velocity_var"]), a["state"], a["state_bytes"],
                                       *[a["sm_" + k] for k in ORDER], a["sm_counts"], a["emit_frame"], a["num_emitted"],
                                       *[a["fc_" + k] for k in ORDER], self.Hh._stream())
        if st == 0 and fill:
            bufs.update(self._fill(bufs, "sm_", R, F))
            if N:
                bufs.update(self._fill(bufs, "fc_", N, Hz))
        torch.cuda.synchronize()
        got, clean = {}, True
        for k, (flat, view, fill_, shp) in bufs.items():
            n = int(np.prod(shp))
            got[k] = view[:n].view(shp).cpu().numpy()
            clean = clean and bool((view[n:] == fill_).all())
        return st, got, clean, {k: v[2] for k, v in bufs.items()}

    def tail(self, fill=True, **kw):
        L, p, S, C, lag = self.L, self.p, self.S, self.C, self.lag
        N = S * lag
        bufs = {"tl_" + k: sentinel(shp, TABLE_DTYPES[k]) + (shp,) for k, shp in table_shapes(C, N).items()}
        bufs["tail_frame"] = sentinel((S, lag), torch.int32) + ((S, lag),)
        a = dict(T=self.T, S=S, C=C, L=lag, D=self.D, max_age=self.max_age, H=IMG[0], W=IMG[1], state=p(self.state),
                 state_bytes=self.state_bytes)
        a.update({k: p(v[1]) for k, v in bufs.items()})
        a.update(kw)
        st = L.air_track_smooth_tail(a["T"], a["S"], a["C"], a["L"], a["D"], a["max_age"], a["H"], a["W"], a["state"], a["state_bytes"],
                                     *[a["tl_" + k] for k in ORDER], a["tail_frame"], self.Hh._stream())
        if st == 0 and fill and N:
            bufs.update(self._fill(bufs, "tl_", N, lag))
        torch.cuda.synchronize()
        got, clean = {}, True
        for k, (flat, view, fill_, shp) in bufs.items():
            n = int(np.prod(shp))
            got[k] = view[:n].view(shp).cpu().numpy()
            clean = clean and bool((view[n:] == fill_).all())
        return st, got, clean, {k: v[2] for k, v in bufs.items()}


def check_outputs(got, ref, prefixes=("sm_", "fc_")):
    for k, w in ref.items():
        if not k.startswith(prefixes) and k not in ("emit_frame", "num_emitted", "sm_counts", "tail_frame"):
            continue
        if w.size == 0 and k not in got:
            continue
        assert same(got[k], w), (k, np.argwhere(got[k] != w)[:4])


def stream_for(case, F, lag, horizon):
    return DeviceStream(case["S"], F, case["T"], case["A"], case["G"], lag, case["max_age"], horizon)


# ---- 1. air_track_smooth_stream (with the stash and the fill) chunk by chunk against the reference --------------------------------------
RAGGED = [np.array(v, np.int64) for v in ([2, 1, 0], [0, 2, 2], [2, 2, 1])]
even = lambda S, F, chunks: [np.full(S, F, np.int64)] * chunks
# key of the case, F_chunk, valid per chunk
SHAPES = {"1,1,1,1,3": ((1, 1, 1, 3, 1), 1, even(1, 1, 3)),
          "3,5,3,2,3-ragged": ((3, 5, 3, 6, 1), 2, RAGGED),
          "6,50,2,5,3-max_age2": ((6, 50, 2, 15, 2), 5, even(2, 5, 3)),
          "32,5,1,2,3-full": ((32, 5, 1, 6, 1), 2, even(1, 2, 3)),
          "3,50,1,1,6": ((3, 50, 1, 6, 1), 1, even(1, 1, 6))}


@pytest.mark.parametrize("horizon", [0, 3])
@pytest.mark.parametrize("lag", ["max_age", 4])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_stream_kernels_are_the_reference(gpu_device, shape, lag, horizon):
    """every output element, the sentinel tails behind every buffer, NaN padding rows with counts of 99 that are never read, and the
    state and the row ring after every chunk by bytes; the tail after every chunk too"""
    key, F, valids = SHAPES[shape]
    case = stream_case(*key)
    lag = case["max_age"] if lag == "max_age" else lag
    dev = stream_for(case, F, lag, horizon)
    state, emitted, filled = None, 0, 0
    for c in cut(case, F, valids, pad="nan"):
        ref, state = push(state, c, lag, horizon)
        st, got, clean, _ = dev.push(c)
        assert st == 0 and clean
        check_outputs(got, ref)
        dev.check_state(state)
        emitted += int(ref["num_emitted"].sum())
        filled += int(ref["sm_counts"][:, FILLED].sum())
        st, got, clean, _ = dev.tail()
        assert st == 0 and clean
        check_outputs(got, trajectory.reference_smooth_tail(state, lag, case["max_age"], IMG), ("tl_",))
        dev.check_state(state)                                     # 4: the tail leaves the state byte-identical
    print("%s lag %d: emitted %d frames, %d filled rows" % (shape, lag, emitted, filled))
    assert emitted == sum(max(0, int(sum(v[s] for v in valids)) - lag) for s in range(case["S"]))
    if key[0] == 32:
        assert dev.C == 32 and (state["slots"][0, trajectory.SM_LIVE] == 1).all()      # all 32 rows live across both boundaries


# ---- 2. device against device: the one-shot kernel -----------------------------------------------------------------------------------------
def test_a_long_lag_plus_the_tail_is_the_one_shot_kernel(gpu_device):
    key, Hz = (3, 5, 3, 6, 1), 3
    case = stream_case(*key)
    S, Ft, lag = case["S"], case["F"], 6
    st, one, clean, _, _ = run_smooth(case, Hz, NOISE)
    assert st == 0 and clean
    for name, F, valids in chunkings(S, Ft)[2:]:                   # twos, fours, ragged with a valid = 0 chunk
        dev = stream_for(case, F, lag, Hz)
        for c in cut(case, F, valids):
            st, got, clean, _ = dev.push(c, fill=False)
            assert st == 0 and clean and (got["num_emitted"] == 0).all() and (got["sm_state"] == ABSENT).all()
        st, tail, clean, _ = dev.tail(fill=False)
        assert st == 0 and clean and (tail["tail_frame"] == np.arange(Ft)[None]).all()
        for k in ORDER:                                            # sequence-major columns, s L + g == s F_total + g
            assert same(tail["tl_" + k], one["sm_" + k]), (name, k)
            assert same(got["fc_" + k], one["fc_" + k]), (name, "fc_" + k)


# ---- 3. the fill across a chunk boundary ---------------------------------------------------------------------------------------------------
def test_fill_takes_rows_of_an_earlier_chunk(gpu_device):
    """F = 2, L = max_age = 1, one track sighted in frames 0, 1, 3: frame 2, the first of the second chunk, is FILLED from frame 1,
    max_age frames before it across the boundary, and emitted by the second push; frame 1 is emitted there too, its source in the
    first chunk.  The forecast after the second push copies frame 3's rows; after the third (frames 4, 5 empty) the track is retired"""
    T, F, A, G = 2, 2, 5, 8
    z = [np.array([0.2, 0.05 * f, 0.25, -0.03 * f], np.float32) for f in range(6)]
    where, n, ids = planted(z, [1, 1, 0, 1, 0, 0])
    rng = np.random.default_rng(2)
    rows = dict(what=rng.normal(size=(T, 6, A)).astype(np.float32), glimpse=rng.uniform(size=(T, 6, G)).astype(np.float32),
                score=rng.uniform(size=(T, 6)).astype(np.float32))
    dev = DeviceStream(1, F, T, A, G, 1, 1, 2)
    state = None
    for i in range(3):
        sl = slice(2 * i, 2 * i + 2)
        c = dict(where=where[:, sl], n=n[sl], track_id=ids[:, sl], valid=np.array([2]), F=F, max_age=1,
                 **{k: v[:, sl] for k, v in rows.items()})
        ref, state = push(state, c, 1, 2)
        st, got, clean, _ = dev.push(c)
        assert st == 0 and clean
        check_outputs(got, ref)
        dev.check_state(state)
        if i == 1:
            assert got["emit_frame"][0].tolist() == [1, 2] and got["sm_state"][0].tolist() == [OBSERVED, FILLED]
            assert got["sm_src_frame"][0].tolist() == [1, 1] and got["sm_src_slot"][0].tolist() == [1, 1]
            for e in range(2):
                assert all(same(got["sm_" + k][0, e], rows[k][1, 1]) for k in ROWS)
                assert got["fc_src_frame"][0, e] == 3 and all(same(got["fc_" + k][0, e], rows[k][1, 3]) for k in ROWS)
        if i == 2:
            assert got["emit_frame"][0].tolist() == [3, 4] and got["sm_count"].tolist() == [1, 0]      # retired: it does not span 4
            assert (got["fc_count"] == 0).all()
    st, got, clean, _ = dev.tail()
    assert st == 0 and clean and got["tail_frame"].tolist() == [[5]] and got["tl_count"].tolist() == [0]


# ---- 4. a push after a tail ---------------------------------------------------------------------------------------------------------------
def test_a_push_after_a_tail_gives_the_bytes_of_a_push_without_it(gpu_device):
    case = stream_case(3, 5, 3, 6, 1)
    chunks = cut(case, 2, RAGGED)
    with_tail, without = stream_for(case, 2, 2, 3), stream_for(case, 2, 2, 3)
    for c in chunks:
        st, a, clean_a, _ = with_tail.push(c)
        st2, b, clean_b, _ = without.push(c)
        assert st == 0 and st2 == 0 and clean_a and clean_b
        assert sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
        before = with_tail.state_host()
        assert with_tail.tail()[0] == 0
        after = with_tail.state_host()
        assert same(before[0], after[0]) and all(same(before[1][k], after[1][k]) for k in ROWS)
        assert same(after[0], without.state_host()[0])


# ---- 7. argument errors before any launch ------------------------------------------------------------------------------------------------
def test_a_refused_call_writes_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case = stream_case(3, 5, 3, 6, 1)
    c = cut(case, 2, RAGGED)[0]
    dev = stream_for(case, 2, 2, 3)
    before = dev.state_host()
    nan = float("nan")
    off = torch.zeros(3 * 6 * 4 + 1, device="cuda")
    for kw, code in ((dict(where=None), -1), (dict(track_id=None), -1), (dict(valid=None), -1), (dict(state=None), -1),
                     (dict(sm_where=None), -1), (dict(emit_frame=None), -1), (dict(num_emitted=None), -1), (dict(fc_boxes=None), -1),
                     (dict(L=0), -2), (dict(L=17), -2), (dict(C=5), -2), (dict(C=7), -2), (dict(T=0), -2), (dict(T=33), -2),
                     (dict(Hz=17), -2), (dict(Hz=-1), -2), (dict(R=7), -2), (dict(S=0), -2), (dict(F=0), -2), (dict(D=4), -2),
                     (dict(D=0), -2), (dict(max_age=-1), -2), (dict(q_shift=0.0), -2), (dict(r=nan), -2), (dict(velocity_var=-1.0), -2),
                     (dict(state_bytes=dev.state_bytes - 8), -4), (dict(state_bytes=0), -4), (dict(where=Hh._p(off[1:])), -3),
                     # outside the supported noise domain (r = 3e-4): velocity_var / r > 1e6, q / r > 1e15, q / r < 1e-29, r out of range
                     (dict(velocity_var=1e6), -2), (dict(velocity_var=301.0), -2), (dict(q_shift=3.1e11), -2), (dict(q_scale=1e-33), -2),
                     (dict(q_shift=1.0, q_scale=1.0, r=3e-17, velocity_var=0.0), -2),
                     (dict(q_shift=1e-300, q_scale=1e-300, r=1e-300, velocity_var=0.0), -2),
                     (dict(q_shift=1e140, q_scale=1e140, r=1e140, velocity_var=1e140), -2)):
        st, got, clean, fill = dev.push(c, **kw)
        assert st == code, (kw, st)
        assert clean and all((got[k] == fill[k]).all() for k in got), kw
    for kw, code in ((dict(state=None), -1), (dict(tl_where=None), -1), (dict(tail_frame=None), -1), (dict(L=0), -2), (dict(L=17), -2),
                     (dict(C=5), -2), (dict(T=33), -2), (dict(D=2), -2), (dict(state_bytes=dev.state_bytes - 8), -4)):
        st, got, clean, fill = dev.tail(**kw)
        assert st == code, (kw, st)
        assert clean and all((got[k] == fill[k]).all() for k in got), kw
    after = dev.state_host()
    assert same(before[0], after[0]) and after[2]
    L = Hh.lib()
    assert L.air_track_smooth_stream_state_bytes(0, 5) == 0 and L.air_track_smooth_stream_state_bytes(3, 0) == 0
    assert L.air_track_stash(None, None, None, None, None, 3, 3, 2, 6, 5, 4, 5, None, None, None, None) == -1
    assert L.air_track_fill_stream(None, None, None, None, None, None, 3, 3, 5, 6, 6, 2, 5, 4, None, None, None, None) == -1
    x = Hh._p(off)
    assert L.air_track_stash(x, x, x, x, x, 3, 3, 2, 7, 5, 4, 5, x, x, x, None) == -2
    assert L.air_track_fill_stream(x, x, x, x, x, x, 3, 3, 5, 6, 7, 2, 5, 4, x, x, x, None) == -2


# ---- 5. StreamSmoother end to end ---------------------------------------------------------------------------------------------------------
PUSHES = ([2, 2, 2], [2, 2, 2], [2, 1, 0])                         # three pushes, the last one ragged
RULE = dict(iou_gate=0.05, birth_score=0.0)                        # (an untrained model's scores are low)


def make_smoother(name, S, F, lag, horizon, capture=False, **kw):
    from test_track_stream import make_stream
    ocfg, tk, ps = make_stream(name, S, F, capture=capture, **kw)
    sm = trajectory.StreamSmoother(tk, lag, horizon, **NOISE)
    if capture:
        sm.capture()
    return ocfg, sm, tk, ps


def host_chunk(sm, tk, valid):
    """the provider's and the tracker's device buffers of the latest push, as a chunk of trajectory_stream_cases"""
    np_ = lambda t: t.detach().cpu().numpy()
    T, R = tk.T, tk.R
    return dict(where=np_(sm._rows["where"]).reshape(T, R, 4), what=np_(sm._rows["what"]).reshape(T, R, -1),
                glimpse=np_(sm._rows["glimpse"]).reshape(T, R, -1), score=np_(sm.provider.score), n=np_(sm.provider.num_objects),
                track_id=np_(tk.track_id), valid=np.asarray(valid, np.int64), F=tk.F, max_age=tk.max_age)


def smoother_pushes(sm, frames, counts, F):
    done = []
    for c, v in enumerate(PUSHES):
        out = sm.push(frames[:, c * F:(c + 1) * F].contiguous(), np.array(v), counts[c])
        sm.synchronize()
        done.append(({k: x.clone() for k, x in out.items() if torch.is_tensor(x)}, host_chunk(sm, sm.tracker, v)))
    return done


def test_stream_smoother_end_to_end(gpu_device):
    from test_track import frames_for
    from test_track_host import moving_gt
    from attend_infer_repeat_amd import track
    from attend_infer_repeat_amd.score import ParseScorer
    S, F, lag, Hz, G = 3, 2, 2, 2, 2
    ocfg, sm, tk, ps = make_smoother("tiny", S, F, lag, Hz, capture=True, **RULE)
    _, eager, _, _ = make_smoother("tiny", S, F, lag, Hz, **RULE)
    T, R, C, img = ocfg.max_steps, S * F, sm.C, tuple(int(v) for v in ocfg.img_size)
    assert sm._graph is not None and eager._graph is None and sm._tail["graph"] is not None and sm.engine is ps.engine
    assert list(sm.segments) == ["stash", "smooth", "fill", "readout", "fill_forecast", "readout_forecast"]      # ONE graph behind the tracker's
    lc = sm.launch_count()
    assert (lc["track_stash"], lc["track_smooth_stream"], lc["track_fill_stream"], lc["parse_render"], lc["tail"]) == (1, 1, 2, 2, 5)
    assert len(sm._plan) == 10 and lc["tracker"] == tk.launch_count()
    rng = np.random.default_rng(9)
    counts = [torch.from_numpy(rng.integers(0, T + 1, R).astype(np.int32)).cuda() for _ in PUSHES]
    frames = frames_for(ocfg, S, F * len(PUSHES), seed=21).cuda()
    done = smoother_pushes(sm, frames, counts, F)
    assert sm.frames_seen.tolist() == tk.frames_seen.tolist() == [6, 5, 4] and sm.state["seq"].tolist() == [[6, 4], [5, 3], [4, 2]]
    keys = [k for k in done[0][0] if k.startswith(("sm_", "fc_")) or k in ("frames_pred", "emit_frame", "num_emitted")]
    assert {"sm_where", "sm_what", "sm_glimpse", "sm_owner", "sm_obj_step", "fc_boxes", "frames_pred", "emit_frame"} <= set(keys)
    # against the host reference on the provider's own rows, chunk by chunk; the score continued over the emitted frames
    state, sstate, n_rows = None, None, 0
    for c, (got, chunk) in enumerate(done):
        ref, state = push(state, chunk, lag, Hz, img)
        for k, w in ref.items():
            assert same(got[k].cpu().numpy().reshape(w.shape), w), (k, c)
        n_rows += int(ref["sm_count"].sum())
        assert got["frames_pred"].shape == (S, Hz) + tuple(ocfg.img_size)
        assert torch.equal(got["frames_pred"].reshape(-1), got["fc_reconstruction"].reshape(-1))      # the renderer's output on the forecast table
    assert n_rows > 0
    # captured equals eager, the state included; then the tail, which moves nothing
    again = smoother_pushes(eager, frames, counts, F)
    for (a, _), (b, _) in zip(done, again):
        for k in keys:
            assert torch.equal(a[k].reshape(-1).view(torch.uint8) if a[k].is_floating_point() else a[k],
                               b[k].reshape(-1).view(torch.uint8) if b[k].is_floating_point() else b[k]), k
    assert torch.equal(sm.packed, eager.packed) and all(torch.equal(sm.rings[k].view(torch.int32), eager.rings[k].view(torch.int32)) for k in ROWS)
    before = sm.packed.clone()
    tail = sm.tail()
    sm.synchronize()
    want = trajectory.reference_smooth_tail(state, lag, tk.max_age, img)
    for k, w in want.items():
        if k != "num_tail":
            assert same(tail[k].cpu().numpy().reshape(w.shape), w), k
    assert torch.equal(sm.packed, before) and tail["tl_owner"].shape[0] == S * lag
    # the emitted frames are a provider: a ParseScorer binds to them
    scorer = ParseScorer(sm.emitted, G)
    assert (scorer.T, scorer.R) == (C, R) and sm.emitted.KIND == "completed" and sm.emitted.where.data_ptr() == sm.sm["where"].data_ptr()
    # a saved state re-runs a chunk to the same bytes; reset([s]) restarts one sequence only; a push behind the back is refused
    sm.load_state_dict(sm.state_dict())
    saved = sm.state_dict()
    chunk = lambda c: frames[:, c * F:(c + 1) * F].contiguous()
    first = {k: v.clone() for k, v in sm.push(chunk(1), np.array(PUSHES[1]), counts[1]).items() if k in keys}
    moved = sm.packed.clone()
    sm.load_state_dict(saved)
    assert sm.frames_seen.tolist() == [6, 5, 4]
    second = sm.push(chunk(1), np.array(PUSHES[1]), counts[1])
    sm.synchronize()
    assert all(torch.equal(first[k].reshape(-1).view(torch.uint8), second[k].reshape(-1).view(torch.uint8)) for k in keys)
    assert torch.equal(sm.packed, moved) and sm.frames_seen.tolist() == [8, 7, 6]
    sm.reset([1])
    sm.synchronize()
    fresh = trajectory.pack_smooth_state(trajectory.new_smooth_state(S, F, lag, tk.max_age, T, sm.A, sm.G))
    now, was = trajectory.unpack_smooth_state(sm.packed.cpu().numpy(), S, sm.depth), trajectory.unpack_smooth_state(moved.cpu().numpy(), S, sm.depth)
    blank = trajectory.unpack_smooth_state(fresh, S, sm.depth)
    for k in trajectory.SMOOTH_STATE_KEYS:
        assert same(now[k][1], blank[k][1]) and same(now[k][[0, 2]], was[k][[0, 2]]), k
    assert sm.frames_seen.tolist() == tk.frames_seen.tolist() == [8, 0, 6] and (sm.rings["what"][1] == 0).all()
    tk.push(chunk(0), None, counts[0])                             # behind the smoother's back
    with pytest.raises(ValueError, match="behind"):
        sm.push(chunk(1), None, counts[1])
    tk.reset()
    with pytest.raises(ValueError, match="behind"):
        sm.push(chunk(1), None, counts[1])
    sm.reset()
    # the score on the emitted frames over three pushes
    sstate = None
    for c, v in enumerate(PUSHES):
        out = sm.push(chunk(c), np.array(v), counts[c])
        sm.synchronize()
        boxes, cnt, ids = (out[k].cpu().numpy() for k in ("sm_boxes", "sm_count", "sm_id"))
        ne = out["num_emitted"].cpu().numpy()
        gt = moving_gt(dict(boxes=boxes, n=cnt, T=C, S=S, F=F), np.random.default_rng(c), G)
        got = sm.score(torch.from_numpy(gt.reshape(S, F, G, 4)))
        sm.synchronize()
        want, sstate = track.reference_score_stream(sstate, boxes, cnt, ids, gt, F, ne.astype(np.int64))
        assert np.array_equal(got["seq_counts"].cpu().numpy(), want["seq_counts"]) and np.array_equal(got["gt_match"].cpu().numpy(), want["gt_match"])
        assert same(got["seq_iou"].cpu().numpy(), want["seq_iou"])
    assert sm.summary()["gt"] == int(want["seq_counts"][:, 0].sum())
    with pytest.raises(ValueError):
        trajectory.StreamSmoother(tk, lag=0)
    with pytest.raises(ValueError):
        trajectory.StreamSmoother(tk, lag=17)
    with pytest.raises(ValueError):
        trajectory.StreamSmoother(tk, lag=2, horizon=17)
    sm.release_graphs()
    tk.release_graphs()


# ---- 6. the model surface -------------------------------------------------------------------------------------------------------------------
def test_track_stream_smooth_on_the_model(gpu_device):
    from test_parse import _mnist_air
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    B, S, T = 8, 2, 3
    air, ts, x, y = _mnist_air(B)
    for _ in range(2):
        ts()
    d = procedural_moving_mnist(S, 6, n_objects=(1, 2), seed=3, n_templates=32, return_annotations=True)
    frames = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    rule = dict(birth_score=0.0, iou_gate=0.05)
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8) if t.is_floating_point() else t
    tensors = lambda out: {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    plain = tensors(air.track_stream(frames[:, :2], **rule))
    none = tensors(air.track_stream(frames[:, :2], reset=True, smooth=None, **rule))      # smooth=None: exactly today's call
    assert sorted(plain) == sorted(none) and all(torch.equal(raw(plain[k]), raw(none[k])) for k in plain) and len(air._trackers) == 1
    smooth = dict(lag=2, horizon=2)
    emitted = {}
    for name, F in (("twos", 2), ("threes", 3)):                   # two chunkings of the same 6 frames
        rows = [dict() for _ in range(S)]
        for c in range(6 // F):
            out = air.track_stream(frames[:, c * F:(c + 1) * F], reset=(c == 0), smooth=smooth, **rule)
            air._engine.synchronize()
            assert set(plain) < set(out) and {"sm_where", "sm_id", "sm_what", "emit_frame", "num_emitted", "fc_where", "frames_pred"} <= set(out)
            assert tuple(out["frames_pred"].shape[:2]) == (S, 2)
            for s in range(S):
                for e in range(int(out["num_emitted"][s])):
                    g = int(out["emit_frame"][s, e])
                    rows[s][g] = {k: raw(out[k][:, s * F + e]).clone() for k in ("sm_where", "sm_boxes", "sm_id", "sm_state", "sm_src_frame",
                                                                               "sm_velocity", "sm_what", "sm_score")}
        assert all(sorted(r) == [0, 1, 2, 3] for r in rows)
        emitted[name] = rows
    sm = air.stream_smoother(S, 3, smooth, **rule)
    from attend_infer_repeat_amd import stacks
    assert sm is air.stream_smoother(S, 3, smooth, **rule) and sm._graph is not None and sm.tracker._graph is not None
    # keys of their own in the tracker cache (MAX_TRACKERS = 2: the plain stream tracker has been dropped)
    assert len(air._trackers) == 2 and all(isinstance(k, stacks.StreamSmoothKey) for k in air._trackers)
    assert stacks.stream_key(air._engine, S, 3, **rule) not in air._trackers
    for s in range(S):
        for g in range(4):
            for k, v in emitted["twos"][s][g].items():
                assert torch.equal(v, emitted["threes"][s][g][k]), (s, g, k)
    assert any((emitted["twos"][s][g]["sm_id"] >= 0).any() for s in range(S) for g in range(4))
    # the evaluation logger behind scripts/multi_mnist.py --track-stream-smooth: the emitted frames of every sequence, scored once each
    import io
    import json
    from attend_infer_repeat_amd.evaluation import make_track_stream_logger
    data = dict(imgs=d["imgs"].astype(np.float32) / 255, boxes=d["boxes"])
    written = io.StringIO()
    acc = make_track_stream_logger(air, data, 1, "test", 3, S, written, smooth=smooth, measure_time=False, **rule)(itr=7)
    rec = json.loads(written.getvalue())
    present = int((np.asarray(d["boxes"])[:, :4, :, 2] > 0).sum())  # lag 2: frames 0..3 of 6 are emitted
    assert rec["data"] == "test_track_stream_smooth" and (rec["lag"], rec["horizon"], rec["chunk_frames"]) == (2, 2, 3) and acc["gt"] == present
    with pytest.raises(ValueError, match="lag"):
        air.track_stream(frames[:, :2], smooth=dict(lag=0), **rule)
    with pytest.raises(ValueError, match="smooth"):
        air.track_stream(frames[:, :2], smooth=dict(window=3), **rule)
