"""GPU test of the one relabel kernel behind air_parse_objects (csrc/parse_kernels.hip: parse_relabel_kernel, declared in
csrc/scene_device.h): air_prune_relabel and air_tile_relabel check their own arguments and launch it, so on inputs both accept they
must write the same bytes -- the bytes of the rule restated in numpy -- and leave everything outside the rule's footprint alone.

The rule: for j < num_objects[r] clipped to 0..T, score[j, r] = obj_score[offsets[r] + j] = score_src[j, r] and
obj_step[offsets[r] + j] = ids[j, r].  Bit copies: the comparison is of bytes, no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, R = 3, 5                                                        # T = C = 3 rows (both entries take it), R = S = 5 images, two waves' worth
COUNTS = np.array([0, 1, 3, -2, 7], np.int32)                      # -2 and 7: the clamp at 0 and the clamp at T


def _inputs():
    rng = np.random.default_rng(11)
    clamped = np.clip(COUNTS, 0, T)
    offsets = np.concatenate([[0], np.cumsum(clamped)]).astype(np.int32)      # the exclusive scan air_parse_objects writes
    src = rng.normal(size=(T, R)).astype(np.float32)
    src[0, 2] = -0.0                                               # a bit copy keeps the sign of a zero
    ids = rng.integers(0, 256, (T, R)).astype(np.int32)
    return clamped, offsets, src, ids


def _primed():
    return dict(score=np.full((T, R), np.nan, np.float32), obj_score=np.full(T * R, np.nan, np.float32),
                obj_step=np.full(T * R, -1, np.int32))


def _run(entry, offsets, src, ids):
    from attend_infer_repeat_amd import hip as Hh
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(v) for k, v in _primed().items()}
    keep = [dev(src), dev(ids), dev(COUNTS), dev(offsets)]
    st = getattr(Hh.lib(), entry)(*[Hh._p(t) for t in keep], T, R, Hh._p(d["score"]), Hh._p(d["obj_score"]), Hh._p(d["obj_step"]),
                                  Hh._stream())
    torch.cuda.synchronize()
    assert st == 0, (entry, st)
    return {k: v.cpu().numpy().tobytes() for k, v in d.items()}


def test_both_entries_write_the_rule_and_nothing_else(gpu_device):
    clamped, offsets, src, ids = _inputs()
    want, touched = _primed(), {k: np.zeros(v.shape, bool) for k, v in _primed().items()}
    for r in range(R):
        n, o = clamped[r], offsets[r]
        want["score"][:n, r] = src[:n, r]
        want["obj_score"][o:o + n] = src[:n, r]
        want["obj_step"][o:o + n] = ids[:n, r]
        touched["score"][:n, r] = True
        touched["obj_score"][o:o + n] = touched["obj_step"][o:o + n] = True
    assert touched["score"].sum() == touched["obj_score"].sum() == touched["obj_step"].sum() == clamped.sum() == 7
    prune, tile = _run("air_prune_relabel", offsets, src, ids), _run("air_tile_relabel", offsets, src, ids)
    primed = _primed()
    for k in ("score", "obj_score", "obj_step"):
        assert prune[k] == tile[k], k                              # one kernel: identical bytes
        assert prune[k] == want[k].tobytes(), k                    # the rule, bit for bit
        got = np.frombuffer(prune[k], primed[k].dtype).reshape(primed[k].shape)
        outside = ~touched[k]
        assert got[outside].tobytes() == primed[k][outside].tobytes(), k      # NaN / -1 wherever the rule writes nothing
