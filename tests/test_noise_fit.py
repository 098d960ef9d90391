"""Group Nf on the GPU: the two kernels of csrc/noise_fit_kernels.hip, one launch at a time through the C ABI, against
trajectory.reference_noise_stats bit for bit (tests/test_noise_fit_host.py holds that restatement to the exact statistics on the CPU),
then trajectory.TrajectoryNoiseFitter and AIRonMNIST.fit_track_noise end to end.  (Run with -m gpu on an MI355X.)

Per launch: every operand is a window of a NaN (integers: -77777) parent, every output a primed window of a sentinel parent, the totals
a window of a sentinel parent; after the launch every parent is compared byte for byte outside what the launch owns, and every output
element is written."""
import ctypes

import numpy as np
import pytest
import torch

import noise_fit_cases as NC
import smoother_cases as SC

from attend_infer_repeat_amd import trajectory

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(gpu_device):
    from attend_infer_repeat_amd import hip as H
    return H.lib()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want, what):
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r != %r" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[:3].tolist(),
                                                                                     got[bad][:3], want[bad][:3])


class Launch:
    """the buffers of one launch on the device and the check of everything the launch must not have touched"""

    def __init__(self):
        self.items = {}

    def _add(self, name, win):
        dev = torch.from_numpy(win.parent.copy()).cuda()
        self.items[name] = (win, dev)
        return ctypes.c_void_p(dev.data_ptr() + win.byte_offset)

    def inp(self, name, values):
        return self._add(name, SC.Window("in", values))

    def out(self, name, shape, dtype):
        return self._add(name, SC.Window("out", shape=shape, dtype=dtype))

    def state(self, name, values):
        return self._add(name, SC.Window("state", values))

    def finish(self):
        torch.cuda.synchronize()
        got = {}
        for name, (win, dev) in self.items.items():
            host = dev.cpu().numpy()
            assert win.outside_changed(host) == 0, "%s: %d bytes changed outside the window" % (name, win.outside_changed(host))
            if win.kind == "out":
                assert win.unwritten(host) == 0, "%s: %d elements left unwritten" % (name, win.unwritten(host))
            if win.kind != "in":
                got[name] = win.inside(host).copy()
        return got


def launch_stats(L, case, shift, scale, nu):
    ln = Launch()
    T, S, F, R, G = case["T"], case["S"], case["F"], case["R"], len(shift)
    arr = ctypes.c_double * G
    st = L.air_track_noise_stats(ln.inp("where", case["where"]), ln.inp("n", case["n"].astype(np.int32)), ln.inp("track_id", case["track_id"]),
                                 ln.inp("num_tracks", case["num_tracks"].astype(np.int32)), ln.inp("track_first", case["track_first"]),
                                 ln.inp("track_last", case["track_last"]), T, S, F, R, G, arr(*shift), arr(*scale), float(nu),
                                 ln.out("q", (S, G, 2), np.float64), ln.out("m", (S, G, 2), np.float64), ln.out("k", (S, G, 2), np.int32),
                                 ln.out("n_out", (S,), np.int32), stream())
    assert st == 0, st
    got = ln.finish()
    got["n"] = got.pop("n_out")
    return got


def launch_reduce(L, stats, totals, accumulate):
    ln = Launch()
    S, G = stats["q"].shape[:2]
    st = L.air_track_noise_reduce(ln.inp("q", stats["q"]), ln.inp("m", stats["m"]), ln.inp("k", stats["k"]), ln.inp("n", stats["n"]), S, G,
                                  int(accumulate), *[ln.state(k, totals[k]) for k in trajectory.TOTAL_KEYS], stream())
    assert st == 0, st
    return ln.finish()


# ---- 8. air_track_noise_stats -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,row", NC.gpu_rows())
def test_Nf_stats_is_the_reference_bit_for_bit(L, name, row):
    """S = 3, T = 3, F = 8 with gaps, one-sighting tracks and a sequence without tracks; tables no tracker writes (skipped tracks,
    clipped counts, an id in two slots); 70 ids in a sequence (two passes of lanes); G = 1, 5, 32; the ratios at the domain's ends"""
    case, (shift, scale, nu) = NC.gpu_case(name), NC.grid_rows()[row]
    got = launch_stats(L, case, shift, scale, nu)
    ref = NC.reference_totals(case, shift, scale, nu)
    for k in ("n", "k", "m", "q"):
        same(got[k], ref[k], "%s/%s %s" % (name, row, k))
    assert int(ref["n"].sum()) > 0 and np.isfinite(ref["q"]).all()
    if name == "lanes2":
        assert case["num_tracks"][0] > 64 and ref["n"][0] == 21 + 2 + 1


# ---- 9. air_track_noise_reduce ------------------------------------------------------------------------------------------------------------------
def test_Nf_reduce_accumulates_restarts_and_carries_beyond_int32(L):
    shift, scale, nu = NC.grid_rows()["g5"]
    a, b = NC.reference_totals(NC.gpu_case("small"), shift, scale, nu), NC.reference_totals(NC.gpu_case("foreign"), shift, scale, nu)
    empty = trajectory.new_noise_totals(5)
    one = launch_reduce(L, a, empty, 1)                            # into totals that hold nothing
    for k in trajectory.TOTAL_KEYS:
        same(one[k], a[k], "first call " + k)
    two = launch_reduce(L, b, one, 1)                              # a second call, accumulated
    want = trajectory.reference_noise_reduce(b["q"], b["m"], b["k"], b["n"], one)
    for k in trajectory.TOTAL_KEYS:
        same(two[k], want[k], "second call " + k)
    assert two["tot_n"][0] == a["n"].sum() + b["n"].sum()
    again = launch_reduce(L, b, two, 0)                            # accumulate = 0 restarts
    for k in trajectory.TOTAL_KEYS:
        same(again[k], b[k], "restart " + k)
    big = dict(two, tot_k=np.full((5, 2), 2 ** 31 - 3, np.int64), tot_n=np.array([2 ** 40 + 7], np.int64))      # planted directly
    far = launch_reduce(L, a, big, 1)
    want = trajectory.reference_noise_reduce(a["q"], a["m"], a["k"], a["n"], big)
    for k in trajectory.TOTAL_KEYS:
        same(far[k], want[k], "beyond int32 " + k)
    assert (far["tot_k"] > 2 ** 31).all() and far["tot_n"][0] == 2 ** 40 + 7 + a["n"].sum()
    g32 = NC.grid_rows()["g32"]
    c = NC.reference_totals(NC.gpu_case("small"), *g32)
    full = {k: np.concatenate([c[k]] * 11) for k in ("q", "m", "k", "n")}      # S = 33, G = 32: every lane of the workgroup
    got = launch_reduce(L, full, trajectory.new_noise_totals(32), 0)
    want = trajectory.reference_noise_reduce(full["q"], full["m"], full["k"], full["n"])
    for k in trajectory.TOTAL_KEYS:
        same(got[k], want[k], "33 sequences, 32 candidates " + k)


# ---- 10. end to end -----------------------------------------------------------------------------------------------------------------------------
def _tables(f):
    """the provider's and the tracker's device buffers the fitter reads, read back"""
    np_ = lambda t: t.detach().cpu().numpy()
    tk = f.tracker
    return dict(where=np_(f._where).reshape(tk.T, tk.R, 4), n=np_(f.provider.num_objects), track_id=np_(tk.track_id), num_tracks=np_(tk.num_tracks),
                track_first=np_(tk.track_first), track_last=np_(tk.track_last), F=tk.F)


def _watched(f, base):
    w = {k: v for k, v in base.items() if torch.is_tensor(v)}
    w.update({"rows_" + k: v for k, v in f.tracker._rows.items() if torch.is_tensor(v)})
    return w


def _raw(t):
    return t.contiguous().reshape(-1).view(torch.uint8).clone() if t.is_floating_point() else t.clone()


def test_Nf_fitter_on_the_model_graph_and_eager_only_read(gpu_device):
    """data.procedural_moving_mnist through an untrained model at S = 2, F = 3: the fitter's totals are the reference on the read-back
    tables bit for bit, graph replay equals eager, nothing the tracker or the provider owns changes, two launches.  (Whether such a
    model yields a track with two sightings is its own business: the fit itself is test_Nf_fit_track_noise_on_planted_rows's.)"""
    from test_parse import _mnist_air
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    air, ts, x, y = _mnist_air(8)
    ts()
    d = procedural_moving_mnist(2, 3, n_objects=(1, 2), seed=5, n_templates=32)
    frames = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    f = air.noise_fitter(2, 3, birth_score=0.0, iou_gate=0.05)
    assert f is air.noise_fitter(2, 3, birth_score=0.0, iou_gate=0.05) and f._graph is not None and f.G == 19
    assert f.launch_count()["track_noise_stats"] + f.launch_count()["track_noise_reduce"] == 2 and len(f._plan) == 2
    f.load_from(air._engine)
    base = f.tracker.track(frames)
    f.synchronize()
    watched = _watched(f, base)
    before = {k: _raw(v) for k, v in watched.items()}
    f.run(accumulate=False)                                        # the graph
    f.synchronize()
    replay = f.read_totals()
    stats = {k: v.cpu().numpy() for k, v in f.stats.items()}
    for k, v in watched.items():
        assert torch.equal(before[k], _raw(v)), k
    ref = NC.reference_totals(_tables(f), f.shift_ratios, f.scale_ratios, f.velocity_ratio)
    for k in ("n", "k", "m", "q"):
        same(stats[k], ref[k], "model " + k)
    for k in trajectory.TOTAL_KEYS:
        same(replay[k], ref[k], "model " + k)
    f.release_graphs()                                             # eager
    f.run(accumulate=False)
    f.synchronize()
    eager = f.read_totals()
    for k in trajectory.TOTAL_KEYS:
        same(eager[k], replay[k], "eager against replay " + k)
    f.run()                                                        # accumulated: twice the tracks
    twice = f.read_totals()
    want = trajectory.reference_noise_reduce(ref["q"], ref["m"], ref["k"], ref["n"], eager)
    for k in trajectory.TOTAL_KEYS:
        same(twice[k], want[k], "two runs " + k)
    with pytest.raises(ValueError, match="zoom"):
        f.fit(zoom=1)
    print("\n  untrained model on procedural frames: %d tracks, %d updates" % (int(_tables(f)["num_tracks"].sum()), int(ref["n"].sum())))
    f.capture()


def test_Nf_fit_track_noise_on_planted_rows(gpu_device):
    """AIRonMNIST.fit_track_noise with planted rows in the provider's buffers (its parse() is wrapped: an untrained model's own parse
    need not hold a track with two sightings) and the REAL tracker on them: the fit is profile_fit of the reference on the read-back
    tables; zoom does not lower the likelihood; `track(frames, smooth=fitted)` runs and is reference_smooth at the fitted terms"""
    from test_parse import _mnist_air
    from test_trajectory import plant
    from trajectory_cases import PLANTED, planted_sequences
    S, F = PLANTED["S"], PLANTED["F"]
    air, ts, x, y = _mnist_air(8)
    ts()
    case, gt, gt_future, gaps = planted_sequences(A=50, G=400)
    frames = torch.zeros(S, F, 50, 50).cuda()

    def wrap(provider):
        inner = provider.parse

        def planted_parse(*args, **kwargs):
            base = inner(*args, **kwargs)
            plant(provider, case)
            return base
        provider.parse = planted_parse

    f = air.noise_fitter(S, F)
    wrap(f.provider)
    fit = air.fit_track_noise(frames)
    assert fit is air.track_noise_fit and f.runs == 1
    tables = _tables(f)
    assert np.array_equal(tables["num_tracks"], case["num_tracks"]) and np.array_equal(tables["where"].view(np.uint32), case["where"].view(np.uint32))
    ref = NC.reference_totals(tables, f.shift_ratios, f.scale_ratios, f.velocity_ratio)
    want = trajectory.profile_fit(ref, f.shift_ratios, f.scale_ratios, f.velocity_ratio)
    for k in trajectory.TOTAL_KEYS:
        same(fit["totals"][k], ref[k], "planted " + k)
    for k in trajectory.FIT_KEYS + ("loglik", "n_innovations", "cell", "on_edge"):
        assert fit[k] == want[k], (k, fit[k], want[k])
    assert np.array_equal(fit["surface"], want["surface"]) and fit["n_innovations"] == 4 * int(ref["n"].sum()) > 0
    zoomed = air.fit_track_noise(frames, zoom=2)
    evaluate = lambda a, b: {k: v for k, v in NC.reference_totals(tables, a, b, f.velocity_ratio).items() if k in trajectory.TOTAL_KEYS}
    want_z = trajectory.fit_with_zoom(evaluate, f.shift_ratios, f.scale_ratios, f.velocity_ratio, zoom=2)
    assert zoomed["loglik"] >= fit["loglik"] and zoomed["loglik"] == want_z["loglik"] and zoomed["cell"] == want_z["cell"]
    assert zoomed["process_noise"] == want_z["process_noise"] and zoomed["measurement_noise"] == want_z["measurement_noise"]
    print("\n  planted rows: cell %s, on_edge %s, r^ %.3g, loglik / N %.4f -> zoomed %.4f" % (fit["cell"], fit["on_edge"], fit["measurement_noise"],
          fit["loglik"] / fit["n_innovations"], zoomed["loglik"] / zoomed["n_innovations"]))
    fitted = {k: fit[k] for k in trajectory.FIT_KEYS}
    sm = air.trajectory_smoother(S, F, fitted)
    wrap(sm.provider)
    out = air.track(frames, smooth=fitted)
    sm.synchronize()
    assert (sm.process_noise, sm.measurement_noise, sm.velocity_var) == (fit["process_noise"], fit["measurement_noise"], fit["velocity_var"])
    want_sm = trajectory.reference_smooth(case["where"], case["n"], case["track_id"], case["num_tracks"], case["track_first"], case["track_last"],
                                          F, sm.max_age, sm.img_size, 0, **fitted)
    for k in ("sm_where", "sm_id", "sm_state", "sm_count", "sm_velocity"):
        got = out[k].cpu().numpy()
        assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got, want_sm[k].view(np.uint32) if got.dtype == np.float32 else want_sm[k]), k
    with pytest.raises(ValueError, match="smooth"):
        air.fit_track_noise(frames, smooth=True)
    with pytest.raises(ValueError, match="FIT_Q_OVER_R_MAX"):
        air.fit_track_noise(frames, shift_ratios=(1e16,), scale_ratios=(1.0,))


def test_training_script_track_fit_noise_option(gpu_device, tmp_path, capsys):
    import json
    import os
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "2", "--log-every", "2", "--save-every", "1000", "--synthetic-samples", "256", "--eval-batches", "1",
                            "--summary-every", "0", "--results-dir", str(tmp_path), "--track-eval", "4:2.5", "--track-fit-noise", "1"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_track_noise_fit"]
    assert [l["step"] for l in rec] == [0, 2] and printed.count("test_track_noise_fit") == 2
    for l in rec:                                                  # (a model of two steps may hold no track with two sightings: then in words)
        assert l["zoom"] == 1 and (isinstance(l.get("refused"), str) or
                                   (l["measurement_noise"] > 0 and l["n_innovations"] > 0 and len(l["process_noise"]) == 2 and
                                    l["loglik_per_innovation"] >= l["loglik_per_innovation_at_defaults"]))
    for bad in (["--track-fit-noise"], ["--track-eval", "4", "--track-fit-noise", "-1"],
                ["--track-eval", "4", "--eval-batches", "2", "--track-fit-noise", "1"]):
        with pytest.raises(SystemExit):
            multi_mnist.main(bad)
