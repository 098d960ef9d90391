"""The provider protocol on the device (stage.py): every owner of a read-out returns, from `parse()` / `run()`, the very tensors it
exposes as public attributes -- what the stages bound behind it, ParseScorer and the tools read."""
import pytest
import torch

from test_parse import e2e_case, make_parser
from test_particle_parse import make_particle_parser

pytestmark = pytest.mark.gpu

ALIASED = ("num_objects", "presence", "score", "boxes", "owner", "offsets", "reconstruction")


def test_results_are_the_public_read_out_attributes(gpu_device):
    from attend_infer_repeat_amd.propose import ParseProposer
    from attend_infer_repeat_amd.prune import ParsePruner
    from attend_infer_repeat_amd.refine import ParseRefiner
    from attend_infer_repeat_amd.temporal import TemporalProposer
    from attend_infer_repeat_amd.tile import TiledSceneParser
    from attend_infer_repeat_amd.track import SequenceTracker
    from attend_infer_repeat_amd.trajectory import TrajectorySmoother
    ocfg, _, params, obs = e2e_case("mnist_b8")
    R, (H, W) = 4, ocfg.img_size
    assert (H, W, ocfg.max_steps) == (50, 50, 3)
    x = obs[:R].cuda()
    ps = make_parser(ocfg, R, params)
    owners = {"scene": ps, "particle": make_particle_parser(ocfg, R, 2, params), "refiner": ParseRefiner(ps, 1, 1e-2, 1e-2),
              "pruner": ParsePruner(ps, "all"), "proposer": ParseProposer(ps, 1, 1), "temporal": TemporalProposer(ps, 2, 1, 1)}
    for name, owner in owners.items():
        out = owner.parse(x)
        owner.synchronize()
        for k in ALIASED:
            assert out[k].data_ptr() == getattr(owner, k).data_ptr() and out[k].shape == getattr(owner, k).shape, (name, k)
        assert owner.rows()["what"].data_ptr() == out["what"].data_ptr(), name
    tiled = TiledSceneParser(ps, (75, 75))                         # 2 x 2 windows: the 4 rows are one scene
    out = tiled.parse(torch.zeros(1, 75, 75).cuda())
    tiled.synchronize()
    for k in ALIASED:
        assert out[k].data_ptr() == getattr(tiled, k).data_ptr() and out[k].shape == getattr(tiled, k).shape, ("tiled", k)
    assert tiled.owner.shape == (1, 75, 75) and "count_prob" not in out
    # the smoother's two tables: the completed one is its provider surface, the forecast one its `fc` table
    sm = TrajectorySmoother(SequenceTracker(ps, 2, birth_score=0.0), horizon=2)
    out = sm.track(x.view(2, 2, H, W))
    sm.synchronize()
    for k in ("presence", "owner", "offsets", "reconstruction"):
        assert out["sm_" + k].data_ptr() == sm.sm[k].data_ptr() and out["fc_" + k].data_ptr() == sm.fc[k].data_ptr(), k
    for attr, key in (("num_objects", "num_objects"), ("presence", "presence"), ("boxes", "boxes_out"), ("owner", "owner")):
        assert getattr(sm, attr).data_ptr() == sm.sm[key].data_ptr() == getattr(sm.completed, attr).data_ptr(), attr
    assert sm.completed.score.data_ptr() == sm.sm["score_out"].data_ptr() and sm.completed.KIND == "completed"
    assert out["frames_pred"].data_ptr() == sm.fc["reconstruction"].data_ptr()
