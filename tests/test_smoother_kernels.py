"""Group Tj on the GPU: the six kernels of csrc/trajectory_kernels.hip, one launch at a time through the C ABI, against the EXACT posterior
mean of the trajectory model (tests/smoother_cases.py: one weighted least-squares problem solved in rationals) and, in the same rows,
against trajectory.reference_smooth / reference_smooth_stream bit for bit, so that a failure says which side moved.  (Run with -m gpu on
an MI355X; tests/test_smoother_cases_host.py holds the cases, the bound and the planted defects on the CPU.)

Per launch: every operand is a window of a NaN (integers: -77777) parent, every output a primed window of a sentinel parent, in-place
state a window of a sentinel parent; after the launch every parent is compared byte for byte outside what the launch owns, and every
output element is written.  A refused call returns its status and writes nothing.
  air_track_smooth        sm_where / fc_where within one float32 ulp of the rounded exact value, sm_velocity / fc_velocity within one unit
                          of 2^-24 max|z| (as pixels per frame), sm_boxes / fc_boxes the bits of the box rule on the device's own
                          `where`, everything the bits of the reference: at the defaults and at every corner of the supported noise
                          domain; 64 frames; gaps of exactly max_age and of max_age + 1; three passes of lanes; a row at and beyond C;
                          tables no tracker writes.
  air_track_smooth_stream, air_track_smooth_tail   the same sequences in chunks of 1, 2 and 5 frames with ragged `valid`: every emitted
                          and every tail column within one ulp of the exact FIXED-LAG posterior and the bits of the reference, the
                          state and the row ring by bytes after every launch.
  air_track_fill, air_track_stash, air_track_fill_stream   bit copies: payload NaNs and -0.0, sources outside the rows, a state byte
                          outside 0..3, every buffer in turn 4 bytes off 16-byte alignment.
The worst ratio per output is printed when the module finishes (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import smoother_cases as SC

from attend_infer_repeat_amd import trajectory
from attend_infer_repeat_amd.tile import scene_boxes
from attend_infer_repeat_amd.trajectory import ABSENT, FILLED, FORECAST, OBSERVED

pytestmark = pytest.mark.gpu
ORDER = ("where", "boxes", "id", "state", "src_frame", "src_slot", "velocity", "count")      # the entries' order per table
DTYPES = dict(where=np.float32, boxes=np.float32, id=np.int32, state=np.int8, src_frame=np.int32, src_slot=np.int32, velocity=np.float32,
              count=np.int32)
ROWS = ("what", "glimpse", "score")
NOISE = SC.noise_rows()
WORST = {}


@pytest.fixture(scope="module")
def L(gpu_device):
    from attend_infer_repeat_amd import hip as H
    return H.lib()


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    print("\n  group Tj, worst error / bound: " + ", ".join("%s %.3g (%s)" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))


def note(key, ratio, what):
    if key not in WORST or ratio > WORST[key][0]:
        WORST[key] = (ratio, what)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def shapes(C, N):
    return dict(where=(C, N, 4), boxes=(C, N, 4), id=(C, N), state=(C, N), src_frame=(C, N), src_slot=(C, N), velocity=(C, N, 2), count=(N,))


def bits(a):
    """the bits of an array: floats as unsigned integers, every NaN the one quiet NaN (the payload of a NaN an operation makes is the
    implementation's; `raw` keeps it where a copy must carry it)"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    u = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
    return np.where(np.isnan(a), u.dtype.type(0x7fc00000), u)


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what, exact_nan=False):
    f = raw if exact_nan else bits
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = f(got) != f(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[:3].tolist())


class Launch:
    """the buffers of one launch on the device and the check of everything the launch must not have touched"""

    def __init__(self):
        self.items = {}

    def _add(self, name, win):
        dev = torch.from_numpy(win.parent.copy()).cuda()
        self.items[name] = (win, dev)
        return ctypes.c_void_p(dev.data_ptr() + win.byte_offset)

    def inp(self, name, values, off=0):
        return self._add(name, SC.Window("in", values, off=off))

    def out(self, name, shape, dtype, off=0):
        return self._add(name, SC.Window("out", shape=shape, dtype=dtype, off=off))

    def state(self, name, values, off=0):
        return self._add(name, SC.Window("state", values, off=off))

    def finish(self, written=True):
        """{name: host array} of the outputs and the state; written=False: a refused call, nothing at all has changed"""
        torch.cuda.synchronize()
        got = {}
        for name, (win, dev) in self.items.items():
            host = dev.cpu().numpy()
            if not written:
                assert np.array_equal(host.view(np.uint8), win.parent.view(np.uint8)), "%s: a refused call wrote" % name
                continue
            assert win.outside_changed(host) == 0, "%s: %d bytes changed outside the window" % (name, win.outside_changed(host))
            if win.kind == "out":
                assert win.unwritten(host) == 0 or win.dtype.kind == "f", "%s: %d elements left unwritten" % (name, win.unwritten(host))
            if win.kind != "in":
                got[name] = win.inside(host).copy()
        return got


# ---------------------------------------------------------------------------------------------------------------
# air_track_smooth
# ---------------------------------------------------------------------------------------------------------------
def smooth_args(case, Hz, noise, ln):
    """the arguments of air_track_smooth by name, every buffer a window"""
    T, S, F, R, max_age = case["T"], case["S"], case["F"], case["R"], case["max_age"]
    C, N = trajectory.completed_rows(T, max_age), S * Hz
    ws_bytes = 28 * 8 * C * R
    a = dict(where=ln.inp("where", case["where"]), n=ln.inp("n", case["n"].astype(np.int32)), track_id=ln.inp("track_id", case["track_id"]),
             num_tracks=ln.inp("num_tracks", case["num_tracks"]), track_first=ln.inp("track_first", case["track_first"]),
             track_last=ln.inp("track_last", case["track_last"]), T=T, S=S, F=F, R=R, C=C, Hz=Hz, max_age=max_age, H=case["img"][0],
             W=case["img"][1], q_shift=noise["process_noise"][0], q_scale=noise["process_noise"][1], r=noise["measurement_noise"],
             velocity_var=noise["velocity_var"], ws=ln.state("ws", np.zeros(ws_bytes // 8)), ws_bytes=ws_bytes)
    for pre, cols in (("sm_", R), ("fc_", N)):
        for k, shp in shapes(C, cols).items():
            a[pre + k] = ln.out(pre + k, shp, DTYPES[k]) if cols else None
    a["sm_counts"] = ln.out("sm_counts", (S, 3), np.int32)
    return a


def call_smooth(L, a):
    return L.air_track_smooth(a["where"], a["n"], a["track_id"], a["num_tracks"], a["track_first"], a["track_last"], a["T"], a["S"], a["F"],
                              a["R"], a["C"], a["Hz"], a["max_age"], a["H"], a["W"], float(a["q_shift"]), float(a["q_scale"]), float(a["r"]),
                              float(a["velocity_var"]), a["ws"], a["ws_bytes"], *[a["sm_" + k] for k in ORDER], a["sm_counts"],
                              *[a["fc_" + k] for k in ORDER], stream())


def smooth(L, case, Hz, noise):
    ln = Launch()
    a = smooth_args(case, Hz, noise, ln)
    st = call_smooth(L, a)
    assert st == 0, st
    got = ln.finish()
    got.pop("ws")
    return got


def check_against_reference(got, ref, Hz, what):
    for pre in ("sm_",) + (("fc_",) if Hz else ()):
        for k in ORDER:
            same(got[pre + k], ref[pre + k], "%s %s%s" % (what, pre, k))
    same(got["sm_counts"], ref["sm_counts"], what + " sm_counts")


def check_boxes(got, pre, img, what):
    """boxes = the box rule on the DEVICE's own where, bit for bit; ABSENT rows hold zeros"""
    live = got[pre + "id"] >= 0
    want = np.where(live[..., None], scene_boxes(got[pre + "where"], img), np.float32(0.0)).astype(np.float32)
    same(got[pre + "boxes"], want, "%s %sboxes" % (what, pre))
    assert (got[pre + "where"][~live] == 0).all() and (got[pre + "state"][~live] == ABSENT).all()


def fill_args(case, table, N, per_seq, ln, off=None, rows=None):
    """air_track_fill's arguments for a table {state, src_frame, src_slot} [C, N]; off: {buffer: elements off alignment}"""
    off, rows = off or {}, rows or case
    T, F, R, A, G = case["T"], case["F"], case["R"], case["A"], case["G"]
    C = table["state"].shape[0]
    return dict(what=ln.inp("what", rows["what"], off.get("what", 0)), glimpse=ln.inp("glimpse", rows["glimpse"], off.get("glimpse", 0)),
                score=ln.inp("score", rows["score"]), state=ln.inp("state", table["state"]), src_frame=ln.inp("src_frame", table["src_frame"]),
                src_slot=ln.inp("src_slot", table["src_slot"]), T=T, F=F, R=R, C=C, N=N, per_seq=per_seq, A=A, G=G,
                out_what=ln.out("out_what", (C, N, A), np.float32, off.get("out_what", 0)),
                out_glimpse=ln.out("out_glimpse", (C, N, G), np.float32, off.get("out_glimpse", 0)),
                out_score=ln.out("out_score", (C, N), np.float32))


def call_fill(L, a):
    return L.air_track_fill(a["what"], a["glimpse"], a["score"], a["state"], a["src_frame"], a["src_slot"], a["T"], a["F"], a["R"], a["C"],
                            a["N"], a["per_seq"], a["A"], a["G"], a["out_what"], a["out_glimpse"], a["out_score"], stream())


def fill(L, case, table, N, per_seq, off=None, rows=None):
    ln = Launch()
    a = fill_args(case, table, N, per_seq, ln, off, rows)
    assert call_fill(L, a) == 0
    return ln.finish()


@pytest.mark.parametrize("name,row", SC.one_shot_rows())
def test_Tj_smooth_is_the_exact_posterior_and_the_reference(L, name, row):
    """first runs on the device: 64 frames of one track (the longest before: 24 frames of one-sighting tracks, 8 of real ones), gaps of
    8 and of max_age + 1 = 9 frames, three passes of lanes, a track with a row at and beyond C, and every noise row but the defaults"""
    case, Hz, noise = SC.one_shot_case(name), SC.ONE_SHOT[name][1], NOISE[row]
    got = smooth(L, case, Hz, noise)
    ref = SC.reference(case, Hz, noise)
    wp, wv, n = SC.check_exact(case, got, Hz, noise)               # first the exact posterior, then the reference: which side moved?
    print("\n  %s / %s: %d rows, position %.3g ulp, velocity %.3g units" % (name, row, n, wp, wv))
    note("where", wp, "%s/%s" % (name, row))
    note("velocity", wv, "%s/%s" % (name, row))
    exact_ok = n > 0 and wp <= 1.0 and wv <= 1.0
    try:
        check_against_reference(got, ref, Hz, name)
    except AssertionError as e:
        raise AssertionError("the device left the reference (exact posterior %s: %.3g ulp, %.3g units): %s"
                             % ("held" if exact_ok else "missed", wp, wv, e))
    assert exact_ok, "the device is the reference, and both miss the exact posterior: %.3g ulp, %.3g units over %d rows" % (wp, wv, n)
    for pre in ("sm_",) + (("fc_",) if Hz else ()):
        check_boxes(got, pre, case["img"], name)
    if Hz:
        assert (got["fc_state"][got["fc_id"] >= 0] == FORECAST).all()
    for pre, N, per_seq in (("sm_", case["R"], case["F"]),) + ((("fc_", case["S"] * Hz, Hz),) if Hz else ()):
        filled = fill(L, case, {k: got[pre + k] for k in ("state", "src_frame", "src_slot")}, N, per_seq)
        for k in ROWS:
            same(filled["out_" + k], ref[pre + k].reshape(filled["out_" + k].shape), "%s %s%s" % (name, pre, k), exact_nan=True)


def _planted(change):
    """the mixed case with its tables changed; `seqs` no longer describes it, so it is compared with the reference alone"""
    base = SC.one_shot_case("mixed")
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    change(case)
    return case


def _ids_no_row_names(c):
    """slots that are read carry ids no table row names: negative, beyond num_tracks, beyond F T.  Their tracks miss the sighting"""
    assert c["n"][3] >= 2 and c["n"][12] >= 1 and c["n"][15] >= 1
    c["track_id"][0, 3], c["track_id"][1, 3], c["track_id"][0, 12], c["track_id"][0, 15] = -5, 30000, 2, 8 * 3


def _two_slots_one_id(c):
    c["track_id"][1, 1] = c["track_id"][0, 1]                      # frame 1 of sequence 0: slots 0 and 1 carry one id, the lowest is read
    c["where"][1, 1] = np.float32(9.0)


PLANTED = {
    "first_after_last": lambda c: c["track_last"].__setitem__((0, 1), 0),
    "last_beyond_F": lambda c: c["track_last"].__setitem__((0, 0), 8),
    "first_negative": lambda c: c["track_first"].__setitem__((1, 0), -1),
    "num_tracks_negative": lambda c: c["num_tracks"].__setitem__(0, -3),
    "num_tracks_beyond_FT": lambda c: c["num_tracks"].__setitem__(1, 8 * 3 + 5),
    "an_id_no_slot_names": lambda c: (c["num_tracks"].__setitem__(1, 3), c["track_first"].__setitem__((1, 2), 2),
                                      c["track_last"].__setitem__((1, 2), 5)),
    "ids_no_row_names": _ids_no_row_names,
    "two_slots_one_id": _two_slots_one_id,
    "counts_beyond_T_and_negative": lambda c: (c["n"].__setitem__(0, 99), c["n"].__setitem__(9, -4)),
}


@pytest.mark.parametrize("name", list(PLANTED) + ["33_lower_ids"])
def test_Tj_smooth_on_tables_no_tracker_writes(L, name):
    """the entry takes any integers: nothing outside the tables is written, every parent keeps its bits (Launch.finish), and the result
    is the reference's, whose behaviour include/air_hip.h pins"""
    case = SC._cap_case() if name == "33_lower_ids" else _planted(PLANTED[name])
    if name == "counts_beyond_T_and_negative":
        case["where"][2, 0] = case["where"][0, 0]                  # (the third slot of frame 0 is read now: T = 3 of the 99)
    Hz = 2
    got = smooth(L, case, Hz, NOISE["defaults"])
    ref = SC.reference(case, Hz, NOISE["defaults"], fills=False)
    check_against_reference(got, ref, Hz, name)
    if name == "an_id_no_slot_names":                              # a track without sightings: FILLED rows from z = 0, source -1
        at = got["sm_id"][:, 8:] == 2
        assert at.sum() == 4 and (got["sm_state"][:, 8:][at] == FILLED).all() and (got["sm_src_frame"][:, 8:][at] == -1).all()
        assert (got["sm_where"][:, 8:][at] == 0).all()
    if name == "33_lower_ids":
        assert (got["sm_id"][:, 1] != 33).all() and got["sm_id"][16, 2] == 33 and got["sm_count"].tolist() == [32, 32, 17]


def _refusals(L, build, call, rows):
    for tag, change, status in rows:
        ln = Launch()
        a = build(ln)
        change(a)
        st = call(L, a)
        assert st == status, (tag, st)
        ln.finish(written=False)


def _off(p, nbytes):
    return ctypes.c_void_p(p.value + nbytes)


def _guard_rows(entry):
    """smoother_cases.SIZE_GUARDS as refusal rows: the products that index with 32 bits (the host test holds the same statuses)"""
    def change(kw):
        def apply(a):
            kw2 = dict(kw)
            k = kw2.pop("misalign", None)
            a.update(kw2)
            if k:
                a[k] = _off(a[k], 2)
        return apply
    return [(what, change(kw), status) for what, kw, status in SC.SIZE_GUARDS[entry]]


def test_Tj_smooth_refusals_no_other_test_reaches(L):
    case = SC.one_shot_case("mixed")
    build = lambda ln: smooth_args(case, 3, NOISE["defaults"], ln)
    rows = [("H=0", lambda a: a.update(H=0), -2), ("W=0", lambda a: a.update(W=0), -2), ("W<0", lambda a: a.update(W=-50), -2)]
    pointers = ["n", "num_tracks", "track_first", "track_last", "sm_boxes", "sm_id", "sm_state", "sm_src_frame", "sm_src_slot", "sm_velocity",
                "sm_count", "sm_counts"] + ["fc_" + k for k in ORDER if k != "boxes"]
    rows += [(k + "=NULL", (lambda a, k=k: a.update({k: None})), -1) for k in pointers]
    for k in ("sm_where", "sm_boxes", "fc_where", "fc_boxes"):      # 16-byte alignment
        rows.append((k + "+8", (lambda a, k=k: a.update({k: _off(a[k], 8)})), -3))
    for k in ("ws", "sm_velocity", "fc_velocity"):                  # 8-byte alignment
        rows.append((k + "+4", (lambda a, k=k: a.update({k: _off(a[k], 4)})), -3))
    for k in ("n", "track_id", "num_tracks", "track_first", "track_last", "sm_id", "sm_src_frame", "sm_src_slot", "sm_count", "sm_counts",
              "fc_id", "fc_src_frame", "fc_src_slot", "fc_count"):  # 4-byte alignment
        rows.append((k + "+2", (lambda a, k=k: a.update({k: _off(a[k], 2)})), -3))
    rows += [(name, (lambda a, kw=kw: a.update(q_shift=kw["process_noise"][0], q_scale=kw["process_noise"][1], r=kw["measurement_noise"],
                                               velocity_var=kw["velocity_var"])), -2) for name, kw in SC.outside_rows().items()]
    _refusals(L, build, call_smooth, rows + _guard_rows("smooth"))


# ---------------------------------------------------------------------------------------------------------------
# air_track_fill, air_track_stash, air_track_fill_stream: bit copies
# ---------------------------------------------------------------------------------------------------------------
NAN_PAYLOAD = np.array([0x7fa00001], np.uint32).view(np.float32)[0]


def _fill_case(A, G, seed):
    """T = 3, F = 4, S = 2, C = 5: provider rows with a payload NaN and -0.0, and a table whose sources run over every edge"""
    rng = np.random.default_rng(seed)
    T, F, S, C = 3, 4, 2, 5
    R = S * F
    rows = dict(what=rng.normal(size=(T, R, A)).astype(np.float32), glimpse=rng.uniform(size=(T, R, G)).astype(np.float32),
                score=rng.uniform(size=(T, R)).astype(np.float32))
    rows["what"][1, 2, 0], rows["what"][1, 2, A - 1], rows["glimpse"][2, 5, G - 1], rows["score"][0, 3] = NAN_PAYLOAD, -0.0, NAN_PAYLOAD, -0.0
    state = rng.integers(0, 4, (C, R)).astype(np.int8)
    sf, sj = rng.integers(0, F, (C, R)).astype(np.int32), rng.integers(0, T, (C, R)).astype(np.int32)
    state[0, :4], sf[0, :4], sj[0, :4] = (1, 2, 3, 7), (2, 2, 2, 2), (1, 1, 1, 1)      # the NaN row under every state, 7 is outside 0..3
    state[1, :6], sf[1, :6], sj[1, :6] = 1, (-1, F, 0, 0, F + 7, -9), (0, 0, -1, T, 0, 0)      # sources outside the rows: zeros
    state[2, 0] = ABSENT
    case = dict(T=T, F=F, S=S, R=R, A=A, G=G, **rows)
    return case, dict(state=state, src_frame=sf, src_slot=sj)


def _fill_expected(case, table, per_seq):
    T, F = case["T"], case["F"]
    C, N = table["state"].shape
    out = {k: np.zeros((C, N) + case[k].shape[2:], np.float32) for k in ROWS}
    for c in range(C):
        for n in range(N):
            sf, sj = int(table["src_frame"][c, n]), int(table["src_slot"][c, n])
            if table["state"][c, n] != ABSENT and 0 <= sf < F and 0 <= sj < T:
                for k in ROWS:
                    out[k][c, n] = case[k][sj, (n // per_seq) * F + sf]
    return out


@pytest.mark.parametrize("A,G", [(4, 16), (7, 9), (4, 9)])
def test_Tj_fill_is_a_bit_copy_on_either_path(L, A, G):
    case, table = _fill_case(A, G, 7 * A + G)
    want = _fill_expected(case, table, case["F"])
    assert raw(want["what"])[0, 0, 0] == 0x7fa00001 and (want["what"][1, :6] == 0).all() and raw(want["what"])[0, 3, 0] == 0x7fa00001
    for off in (None, dict(what=1), dict(glimpse=1), dict(out_what=1), dict(out_glimpse=1), dict(what=1, glimpse=1, out_what=1, out_glimpse=1)):
        got = fill(L, case, table, case["R"], case["F"], off)       # (a buffer off alignment: the word path, the bits of the vector path)
        for k in ROWS:
            same(got["out_" + k], want[k], "fill %s off %s" % (k, off), exact_nan=True)


def test_Tj_fill_refusals(L):
    case, table = _fill_case(4, 16, 1)
    build = lambda ln: fill_args(case, table, case["R"], case["F"], ln)
    rows = [(k + "=NULL", (lambda a, k=k: a.update({k: None})), -1)
            for k in ("what", "glimpse", "score", "state", "src_frame", "src_slot", "out_what", "out_glimpse", "out_score")]
    rows += [("%s=%d" % (k, v), (lambda a, k=k, v=v: a.update({k: v})), -2)
             for k, v in (("T", 0), ("T", 33), ("C", 0), ("C", 33), ("F", 0), ("R", 0), ("N", 0), ("per_seq", 0), ("A", 0), ("G", 0), ("F", 3),
                          ("per_seq", 3), ("N", 4), ("R", -8), ("A", -4))]
    rows += [(k + "+2", (lambda a, k=k: a.update({k: _off(a[k], 2)})), -3)
             for k in ("what", "glimpse", "score", "src_frame", "src_slot", "out_what", "out_glimpse", "out_score")]
    _refusals(L, build, call_fill, rows + _guard_rows("fill"))


def stash_args(case, valid, seq, D, rings, ln, off=None):
    off = off or {}
    return dict(what=ln.inp("what", case["what"], off.get("what", 0)), glimpse=ln.inp("glimpse", case["glimpse"], off.get("glimpse", 0)),
                score=ln.inp("score", case["score"]), valid=ln.inp("valid", np.asarray(valid, np.int32)), state=ln.inp("seq", seq),
                T=case["T"], S=case["S"], F=case["F"], R=case["R"], A=case["A"], G=case["G"], D=D,
                ring_what=ln.state("ring_what", rings["what"], off.get("ring_what", 0)),
                ring_glimpse=ln.state("ring_glimpse", rings["glimpse"], off.get("ring_glimpse", 0)),
                ring_score=ln.state("ring_score", rings["score"]))


def call_stash(L, a):
    return L.air_track_stash(a["what"], a["glimpse"], a["score"], a["valid"], a["state"], a["T"], a["S"], a["F"], a["R"], a["A"], a["G"],
                             a["D"], a["ring_what"], a["ring_glimpse"], a["ring_score"], stream())


def _rings(case, D, seed=0):
    rng = np.random.default_rng(seed)
    S, T = case["S"], case["T"]
    return dict(what=rng.normal(size=(S, D, T, case["A"])).astype(np.float32), glimpse=rng.normal(size=(S, D, T, case["G"])).astype(np.float32),
                score=rng.normal(size=(S, D, T)).astype(np.float32))


@pytest.mark.parametrize("A,G", [(4, 16), (7, 9)])
def test_Tj_stash_is_a_bit_copy_on_either_path(L, A, G):
    case, _ = _fill_case(A, G, 3 * A + G)
    D, S, F, T = 7, case["S"], case["F"], case["T"]
    rings = _rings(case, D)
    for valid, seen in (([4, 2], [5, 12]), ([9, -1], [0, 3]), ([0, 4], [20, 6]), ([4, 4], [-1, 2])):      # (frames_seen < 0: nothing)
        seq = np.array([[seen[0], 0], [seen[1], 0]], np.int32)
        want = {k: v.copy() for k, v in rings.items()}
        for s in range(S):
            for f in range(min(max(valid[s], 0), F) if seen[s] >= 0 else 0):
                for k in ROWS:
                    want[k][s, (seen[s] + f) % D] = case[k][:, s * F + f]
        if seen[0] == 5:                                           # the payload NaN of slot 1, frame 2 lands in ring frame (5 + 2) mod 7
            assert raw(want["what"])[0, 0, 1, 0] == 0x7fa00001
        for off in (None, dict(what=1), dict(glimpse=1), dict(ring_what=1), dict(ring_glimpse=1)):
            ln = Launch()
            assert call_stash(L, stash_args(case, valid, seq, D, rings, ln, off)) == 0
            got = ln.finish()
            for k in ROWS:
                same(got["ring_" + k], want[k], "stash %s valid %s off %s" % (k, valid, off), exact_nan=True)


def test_Tj_stash_refusals(L):
    case, _ = _fill_case(4, 16, 2)
    rings, seq = _rings(case, 7), np.zeros((2, 2), np.int32)
    build = lambda ln: stash_args(case, [4, 4], seq, 7, rings, ln)
    rows = [(k + "=NULL", (lambda a, k=k: a.update({k: None})), -1)
            for k in ("what", "glimpse", "score", "valid", "state", "ring_what", "ring_glimpse", "ring_score")]
    rows += [("%s=%d" % (k, v), (lambda a, k=k, v=v: a.update({k: v})), -2)
             for k, v in (("T", 0), ("T", 33), ("S", 0), ("F", 0), ("A", 0), ("G", 0), ("D", 0), ("R", 7), ("S", 3))]
    rows += [(k + "+2", (lambda a, k=k: a.update({k: _off(a[k], 2)})), -3)
             for k in ("what", "glimpse", "score", "valid", "state", "ring_what", "ring_glimpse", "ring_score")]
    _refusals(L, build, call_stash, rows + _guard_rows("stash"))


def fill_stream_args(case, rings, table, D, N, per_seq, ln, off=None):
    off = off or {}
    C = table["state"].shape[0]
    return dict(ring_what=ln.inp("ring_what", rings["what"], off.get("ring_what", 0)),
                ring_glimpse=ln.inp("ring_glimpse", rings["glimpse"], off.get("ring_glimpse", 0)), ring_score=ln.inp("ring_score", rings["score"]),
                state=ln.inp("state", table["state"]), src_frame=ln.inp("src_frame", table["src_frame"]),
                src_slot=ln.inp("src_slot", table["src_slot"]), T=case["T"], S=case["S"], D=D, C=C, N=N, per_seq=per_seq, A=case["A"], G=case["G"],
                out_what=ln.out("out_what", (C, N, case["A"]), np.float32, off.get("out_what", 0)),
                out_glimpse=ln.out("out_glimpse", (C, N, case["G"]), np.float32, off.get("out_glimpse", 0)),
                out_score=ln.out("out_score", (C, N), np.float32))


def call_fill_stream(L, a):
    return L.air_track_fill_stream(a["ring_what"], a["ring_glimpse"], a["ring_score"], a["state"], a["src_frame"], a["src_slot"], a["T"],
                                   a["S"], a["D"], a["C"], a["N"], a["per_seq"], a["A"], a["G"], a["out_what"], a["out_glimpse"],
                                   a["out_score"], stream())


def fill_stream(L, case, rings, table, D, N, per_seq, off=None):
    ln = Launch()
    assert call_fill_stream(L, fill_stream_args(case, rings, table, D, N, per_seq, ln, off)) == 0
    return ln.finish()


@pytest.mark.parametrize("A,G", [(4, 16), (7, 9)])
def test_Tj_fill_stream_is_a_bit_copy_on_either_path(L, A, G):
    case, table = _fill_case(A, G, 5 * A + G)
    D, S, T, F = 7, case["S"], case["T"], case["F"]
    rings = _rings(case, D, 1)
    rings["what"][0, 2, 1, 0], rings["what"][0, 2, 1, A - 1], rings["score"][1, 3, 0] = NAN_PAYLOAD, -0.0, -0.0
    table = {k: v.copy() for k, v in table.items()}
    table["src_frame"][3] = np.arange(case["R"]) + 5 * D + 2       # a GLOBAL frame several multiples of D behind the ring's head
    table["src_frame"][0, :4], table["src_slot"][0, :4] = 2 + 3 * D, 1
    table["state"][3] = OBSERVED
    C, N = table["state"].shape
    want = {k: np.zeros((C, N) + rings[k].shape[3:], np.float32) for k in ROWS}
    for c in range(C):
        for n in range(N):
            sf, sj = int(table["src_frame"][c, n]), int(table["src_slot"][c, n])
            if table["state"][c, n] != ABSENT and sf >= 0 and 0 <= sj < T:      # (a global frame has no upper edge)
                for k in ROWS:
                    want[k][c, n] = rings[k][n // F, sf % D, sj]
    assert raw(want["what"])[0, 3, 0] == 0x7fa00001 and (want["what"][1, 0] == 0).all() and (want["what"][1, 2:4] == 0).all()
    for off in (None, dict(ring_what=1), dict(ring_glimpse=1), dict(out_what=1), dict(out_glimpse=1)):
        got = fill_stream(L, case, rings, table, D, N, F, off)
        for k in ROWS:
            same(got["out_" + k], want[k], "fill_stream %s off %s" % (k, off), exact_nan=True)


def test_Tj_fill_stream_refusals(L):
    case, table = _fill_case(4, 16, 4)
    rings = _rings(case, 7)
    build = lambda ln: fill_stream_args(case, rings, table, 7, case["R"], case["F"], ln)
    rows = [(k + "=NULL", (lambda a, k=k: a.update({k: None})), -1)
            for k in ("ring_what", "ring_glimpse", "ring_score", "state", "src_frame", "src_slot", "out_what", "out_glimpse", "out_score")]
    rows += [("%s=%d" % (k, v), (lambda a, k=k, v=v: a.update({k: v})), -2)
             for k, v in (("T", 0), ("T", 33), ("C", 0), ("C", 33), ("S", 0), ("D", 0), ("N", 0), ("per_seq", 0), ("A", 0), ("G", 0),
                          ("per_seq", 3), ("S", 3), ("N", 12))]
    rows += [(k + "+2", (lambda a, k=k: a.update({k: _off(a[k], 2)})), -3)
             for k in ("ring_what", "ring_glimpse", "ring_score", "src_frame", "src_slot", "out_what", "out_glimpse", "out_score")]
    _refusals(L, build, call_fill_stream, rows + _guard_rows("fill_stream"))


# ---------------------------------------------------------------------------------------------------------------
# air_track_smooth_stream, air_track_smooth_tail
# ---------------------------------------------------------------------------------------------------------------
def stream_args(case, c, F, lag, Hz, noise, packed, ln, D=None):
    T, S, max_age = case["T"], case["S"], case["max_age"]
    C, R, N = trajectory.completed_rows(T, max_age), S * F, S * Hz
    D = trajectory.ring_depth(F, lag, max_age) if D is None else D
    a = dict(where=ln.inp("where", c["where"]), n=ln.inp("n", c["n"]), track_id=ln.inp("track_id", c["track_id"]),
             valid=ln.inp("valid", c["valid"]), T=T, S=S, F=F, R=R, C=C, L=lag, Hz=Hz, D=D, max_age=max_age, H=case["img"][0], W=case["img"][1],
             q_shift=noise["process_noise"][0], q_scale=noise["process_noise"][1], r=noise["measurement_noise"],
             velocity_var=noise["velocity_var"], state=ln.state("state", packed), state_bytes=packed.size)
    for pre, cols in (("sm_", R), ("fc_", N)):
        for k, shp in shapes(C, cols).items():
            a[pre + k] = ln.out(pre + k, shp, DTYPES[k]) if cols else None
    for k, shp in (("sm_counts", (S, 3)), ("emit_frame", (S, F)), ("num_emitted", (S,))):
        a[k] = ln.out(k, shp, np.int32)
    return a


def call_stream(L, a):
    return L.air_track_smooth_stream(a["where"], a["n"], a["track_id"], a["valid"], a["T"], a["S"], a["F"], a["R"], a["C"], a["L"], a["Hz"],
                                     a["D"], a["max_age"], a["H"], a["W"], float(a["q_shift"]), float(a["q_scale"]), float(a["r"]),
                                     float(a["velocity_var"]), a["state"], a["state_bytes"], *[a["sm_" + k] for k in ORDER], a["sm_counts"],
                                     a["emit_frame"], a["num_emitted"], *[a["fc_" + k] for k in ORDER], stream())


def tail_args(case, lag, packed, ln, D):
    T, S, max_age = case["T"], case["S"], case["max_age"]
    C = trajectory.completed_rows(T, max_age)
    a = dict(T=T, S=S, C=C, L=lag, D=D, max_age=max_age, H=case["img"][0], W=case["img"][1], state=ln.inp("state", packed),
             state_bytes=packed.size)
    for k, shp in shapes(C, S * max(lag, 1)).items():
        a["tl_" + k] = ln.out("tl_" + k, shp, DTYPES[k])
    a["tail_frame"] = ln.out("tail_frame", (S, max(lag, 1)), np.int32)
    return a


def call_tail(L, a):
    return L.air_track_smooth_tail(a["T"], a["S"], a["C"], a["L"], a["D"], a["max_age"], a["H"], a["W"], a["state"], a["state_bytes"],
                                   *[a["tl_" + k] for k in ORDER], a["tail_frame"], stream())


def check_table(got, ref, pre, what):
    for k in ORDER:
        same(got[pre + k], ref[pre + k], "%s %s%s" % (what, pre, k))


@pytest.mark.parametrize("F,lag,Hz,row", SC.STREAMS)
def test_Tj_stream_is_the_exact_fixed_lag_posterior_and_the_reference(L, F, lag, Hz, row):
    """the planted sequences in chunks with ragged valid (0, less than F, negative, above F), D exactly F + L + max_age so the ring
    wraps; per push the stash, the smoother, the fills of both tables and the tail, each its own launch.  L = 16 >= the 12 frames:
    nothing is emitted and the tail after the last push is the one-shot exact posterior"""
    case, noise = SC.stream_sequences(), NOISE[row]
    S, T, A, G, max_age = case["S"], case["T"], case["A"], case["G"], case["max_age"]
    D, C = trajectory.ring_depth(F, lag, max_age), trajectory.completed_rows(T, max_age)
    chunks = SC.stream_chunks(case, F, SC.ragged_valids(S, F, case["F"]))
    refs = SC.stream_reference(case, F, lag, Hz, noise, chunks)
    fresh = trajectory.new_smooth_state(S, F, lag, max_age, T, A, G)
    packed, rings = trajectory.pack_smooth_state(fresh), {k: fresh[k] for k in ROWS}
    assert L.air_track_smooth_stream_state_bytes(S, D) == packed.size
    worst_p = worst_v = 0.0
    rows_checked = emitted = 0
    for i, (c, (ref, ref_state, ref_tail)) in enumerate(zip(chunks, refs)):
        what = "F %d L %d push %d" % (F, lag, i)
        ln = Launch()                                              # ---- the stash, before frames_seen moves
        chunk_rows = dict(case, F=F, R=S * F, what=c["what"], glimpse=c["glimpse"], score=c["score"])
        seq = trajectory.unpack_smooth_state(packed, S, D)["seq"]
        assert call_stash(L, stash_args(chunk_rows, c["valid"], seq, D, rings, ln)) == 0
        got = ln.finish()
        rings = {k: got["ring_" + k] for k in ROWS}
        for k in ROWS:
            same(rings[k], ref_state[k], what + " ring " + k, exact_nan=True)
        ln = Launch()                                              # ---- the smoother
        assert call_stream(L, stream_args(case, c, F, lag, Hz, noise, packed, ln)) == 0
        got = ln.finish()
        packed = got.pop("state")
        wp, wv, n = SC.check_stream_exact(case, F, lag, Hz, noise, c, got, None)
        worst_p, worst_v, rows_checked = max(worst_p, wp), max(worst_v, wv), rows_checked + n
        check_table(got, ref, "sm_", what)
        if Hz:
            check_table(got, ref, "fc_", what)
            check_boxes(got, "fc_", case["img"], what)
        check_boxes(got, "sm_", case["img"], what)
        for k in ("sm_counts", "emit_frame", "num_emitted"):
            same(got[k], ref[k], what + " " + k)
        emitted += int(got["num_emitted"].sum())
        same(packed, trajectory.pack_smooth_state(ref_state), what + " state")
        for pre, N, per_seq in (("sm_", S * F, F),) + ((("fc_", S * Hz, Hz),) if Hz else ()):      # ---- the fills from the ring
            filled = fill_stream(L, case, rings, {k: got[pre + k] for k in ("state", "src_frame", "src_slot")}, D, N, per_seq)
            for k in ROWS:
                same(filled["out_" + k], ref[pre + k].reshape(filled["out_" + k].shape), "%s %s%s" % (what, pre, k), exact_nan=True)
        ln = Launch()                                              # ---- the tail: the state is only read (an operand window)
        assert call_tail(L, tail_args(case, lag, packed, ln, D)) == 0
        tail = ln.finish()
        check_table(tail, ref_tail, "tl_", what)
        same(tail["tail_frame"], ref_tail["tail_frame"], what + " tail_frame")
        wp, wv, n = SC.check_stream_exact(case, F, lag, 0, noise, c, dict(got, num_emitted=np.zeros(S, np.int32)), tail)
        worst_p, worst_v, rows_checked = max(worst_p, wp), max(worst_v, wv), rows_checked + n
    print("\n  stream F %d L %d Hz %d %s: %d rows, position %.3g ulp, velocity %.3g units" % (F, lag, Hz, row, rows_checked, worst_p, worst_v))
    note("stream where", worst_p, "F%d L%d %s" % (F, lag, row))
    note("stream velocity", worst_v, "F%d L%d %s" % (F, lag, row))
    assert rows_checked > 50 and worst_p <= 1.0 and worst_v <= 1.0
    assert emitted == S * max(0, case["F"] - lag)
    if lag >= case["F"]:                                           # the stream plus the tail is the one-shot exact posterior
        one = SC.reference(case, 0, noise, fills=False)
        for s in range(S):
            for g in range(case["F"]):
                col = s * lag + (g - max(0, case["F"] - lag))
                for k in ("where", "boxes", "id", "state", "velocity"):
                    same(tail["tl_" + k][:, col], one["sm_" + k][:, s * case["F"] + g], "one-shot %s frame %d" % (k, g))


def test_Tj_tail_of_a_stream_that_has_seen_nothing_and_a_lag_of_zero(L):
    case = SC.stream_sequences()
    S, T, max_age = case["S"], case["T"], case["max_age"]
    F, lag = 2, 4
    D = trajectory.ring_depth(F, lag, max_age)
    packed = trajectory.pack_smooth_state(trajectory.new_smooth_state(S, F, lag, max_age, T, case["A"], case["G"]))
    ln = Launch()
    assert call_tail(L, tail_args(case, lag, packed, ln, D)) == 0
    tail = ln.finish()                                             # b = 0: every row ABSENT, every element written
    assert (tail["tl_state"] == ABSENT).all() and (tail["tl_id"] == -1).all() and (tail["tl_count"] == 0).all()
    assert (tail["tail_frame"] == -1).all() and (tail["tl_where"] == 0).all() and (tail["tl_src_frame"] == -1).all()
    zero = dict(case, max_age=0)                                   # L = 0 (max_age = 0): AIR_OK, nothing is written
    packed = trajectory.pack_smooth_state(trajectory.new_smooth_state(S, F, 0, 0, T, case["A"], case["G"]))
    ln = Launch()
    assert call_tail(L, tail_args(zero, 0, packed, ln, trajectory.ring_depth(F, 0, 0))) == 0
    ln.finish(written=False)


def test_Tj_stream_and_tail_refusals_no_other_test_reaches(L):
    case, noise = SC.stream_sequences(), NOISE["defaults"]
    S, T, max_age, F, lag, Hz = case["S"], case["T"], case["max_age"], 2, 4, 3
    D = trajectory.ring_depth(F, lag, max_age)
    c = SC.stream_chunks(case, F, SC.ragged_valids(S, F, case["F"]))[0]
    packed = trajectory.pack_smooth_state(trajectory.new_smooth_state(S, F, lag, max_age, T, case["A"], case["G"]))
    build = lambda ln: stream_args(case, c, F, lag, Hz, noise, packed, ln)
    rows = [(k + "=NULL", (lambda a, k=k: a.update({k: None})), -1)
            for k in ["n", "sm_counts"] + ["sm_" + k for k in ORDER if k != "where"] + ["fc_" + k for k in ORDER if k != "boxes"]]
    rows += [("%s=%d" % (k, v), (lambda a, k=k, v=v: a.update({k: v})), -2) for k, v in (("H", 0), ("W", 0), ("L", 1), ("D", F + lag + max_age - 1))]
    for k in ("sm_where", "sm_boxes", "fc_where", "fc_boxes"):
        rows.append((k + "+8", (lambda a, k=k: a.update({k: _off(a[k], 8)})), -3))
    for k in ("sm_velocity", "fc_velocity", "state"):
        rows.append((k + "+4", (lambda a, k=k: a.update({k: _off(a[k], 4)})), -3))
    for k in ("n", "track_id", "valid", "sm_id", "sm_src_frame", "sm_src_slot", "sm_count", "sm_counts", "emit_frame", "num_emitted", "fc_id",
              "fc_src_frame", "fc_src_slot", "fc_count"):
        rows.append((k + "+2", (lambda a, k=k: a.update({k: _off(a[k], 2)})), -3))
    rows += [(name, (lambda a, kw=kw: a.update(q_shift=kw["process_noise"][0], q_scale=kw["process_noise"][1], r=kw["measurement_noise"],
                                               velocity_var=kw["velocity_var"])), -2) for name, kw in SC.outside_rows().items()]
    _refusals(L, build, call_stream, rows + _guard_rows("stream"))
    build = lambda ln: tail_args(case, lag, packed, ln, D)
    rows = [("tl_%s=NULL" % k, (lambda a, k=k: a.update({"tl_" + k: None})), -1) for k in ORDER if k != "where"]
    rows += [("%s=%d" % (k, v), (lambda a, k=k, v=v: a.update({k: v})), -2)
             for k, v in (("H", 0), ("W", 0), ("S", 0), ("T", 0), ("max_age", -1), ("L", 1), ("D", 0), ("D", lag + max_age - 1))]
    rows += [("state_bytes=0", lambda a: a.update(state_bytes=0), -4), ("state+4", lambda a: a.update(state=_off(a["state"], 4)), -3)]
    for k, nbytes in (("tl_where", 8), ("tl_boxes", 8), ("tl_velocity", 4), ("tl_id", 2), ("tl_src_frame", 2), ("tl_src_slot", 2), ("tl_count", 2),
                      ("tail_frame", 2)):
        rows.append(("%s+%d" % (k, nbytes), (lambda a, k=k, nbytes=nbytes: a.update({k: _off(a[k], nbytes)})), -3))
    _refusals(L, build, call_tail, rows)
