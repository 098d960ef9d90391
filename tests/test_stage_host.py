"""stage.BoundStage on the host: the plan's life cycle against a stub engine and a stub provider (no device), and which provider
kinds every stage binds to."""
import types

import pytest

from attend_infer_repeat_amd import stage
from attend_infer_repeat_amd.propose import ParseProposer
from attend_infer_repeat_amd.prune import ParsePruner
from attend_infer_repeat_amd.refine import ParseRefiner
from attend_infer_repeat_amd.temporal import TemporalProposer
from attend_infer_repeat_amd.tile import TiledSceneParser
from attend_infer_repeat_amd.track import SequenceTracker


class Engine:
    def __init__(self, log):
        self.cfg, self.log, self.captured = types.SimpleNamespace(output_multiplier=1.0, output_std=0.3, guard_eps=0.0), log, 0

    def synchronize(self):
        self.log.append("synchronize")

    def _capture_plans(self, plans):
        self.captured += 1
        self.log.append("capture")
        return "graph%d" % self.captured


class Provider:
    KIND = "scene"

    def __init__(self, engine, log):
        self.engine, self.log, self.changes = engine, log, True

    def rows(self):
        return {"what": "rows of the provider"}

    def update_config(self, **changes):
        self.log.append("provider.update_config")
        for k, v in changes.items():
            setattr(self.engine.cfg, k, v)
        return self.changes

    def load_from(self, other):
        self.log.append("provider.load_from")


class Stage(stage.BoundStage):
    ACCEPTS = ("scene",)
    KEY_FIELDS = ("output_multiplier", "output_std")

    def __init__(self, provider, log):
        self._start = self.bind(provider)
        self._bound, self.engine, self.log, self.builds, self.entries = provider, provider.engine, log, 0, []
        self._rebuild()

    def _build_plan(self):
        self.builds += 1
        self._plan = [("fn", (self.engine.cfg.output_multiplier,), "entry")]

    def _score_entries(self):
        return self.entries


@pytest.fixture
def bound(monkeypatch):
    log = []
    monkeypatch.setattr(stage, "destroy_graphs", lambda graphs: log.append(("destroy", [g for g in graphs if g is not None])))
    return Stage(Provider(Engine(log), log), log), log


def test_refresh_plan_rebuilds_on_a_key_field_and_recaptures_only_a_held_graph(bound):
    st, log = bound
    assert st._built_for == (1.0, 0.3) and st.builds == 1 and st._graph is None
    assert st._refresh_plan() is False and st.builds == 1
    st.engine.cfg.guard_eps = 1e-3                                 # no KEY_FIELD: nothing to rebuild
    assert st._refresh_plan() is False and st.builds == 1
    st.engine.cfg.output_std = 0.5
    assert st._refresh_plan() is True and st.builds == 2 and st._built_for == (1.0, 0.5)
    assert st._graph is None and "capture" not in log             # no graph was held: none is captured
    assert st._plan[0][1] == (1.0,)
    st.capture()
    assert st._graph == "graph1"
    st.engine.cfg.output_multiplier = 2.0
    assert st._refresh_plan() is True and st.builds == 3 and st._graph == "graph2" and st._plan[0][1] == (2.0,)
    assert ("destroy", ["graph1"]) in log
    assert st._refresh_plan() is False and st._graph == "graph2"


def test_update_config_reports_either_change_and_synchronises_before_a_held_graph_goes(bound):
    st, log = bound
    st._bound.changes = False
    assert st.update_config(guard_eps=1e-3) is False               # neither the provider nor the plan
    assert st.update_config(output_std=0.4) is True and st.builds == 2          # the plan alone
    st._bound.changes = True
    assert st.update_config(guard_eps=2e-3) is True and st.builds == 2          # the provider alone
    assert "synchronize" not in log                                # no graph held: nothing to wait for
    st.capture()
    del log[:]
    assert st.update_config(output_multiplier=3.0) is True
    order = [e if isinstance(e, str) else e[0] for e in log]
    assert order[:2] == ["synchronize", "provider.update_config"]
    assert order.index("synchronize") < order.index("destroy") < order.index("capture")
    assert ("destroy", ["graph1"]) in log and st._graph == "graph2"
    del log[:]
    st.load_from(None)                                             # forwards, then looks at the plan
    assert log == ["provider.load_from"] and st.builds == 3


def test_release_graphs_is_idempotent_and_covers_the_score_entries(bound):
    st, log = bound
    st.entries = [{"plan": ["a"], "graph": None}, {"plan": ["b"], "graph": None}]
    st.capture()
    assert st._graph == "graph1" and [e["graph"] for e in st.entries] == ["graph2", "graph3"]
    del log[:]
    st.release_graphs()
    assert log == [("destroy", ["graph1", "graph2", "graph3"])]
    assert st._graph is None and [e["graph"] for e in st.entries] == [None, None]
    st.release_graphs()
    assert log[-1] == ("destroy", []) and st._graph is None


# which kinds a stage binds to; a TrajectorySmoother binds to a SequenceTracker and reads the rows that tracker bound
ACCEPTED = {ParseRefiner: {"scene", "particle"},
            ParsePruner: {"scene", "particle", "refiner"},
            ParseProposer: {"scene", "particle", "refiner"},
            TemporalProposer: {"scene", "refiner", "subset"},
            TiledSceneParser: {"scene", "refiner", "subset"},
            SequenceTracker: {"scene", "refiner", "subset", "tiled"}}
REFUSAL_TEXT = {
    (TemporalProposer, "particle"): "a ParticleParser is out of scope for temporal proposals (its rows are particles of an image, not "
                                    "images): bind a SceneParser, ParseRefiner, ParsePruner or ParseProposer",
    (TemporalProposer, "tiled"): "a TiledSceneParser is out of scope for temporal proposals (its rows are scene slots, up to 32, and "
                                 "the subset search stops at 6 rows): bind a SceneParser, ParseRefiner, ParsePruner or ParseProposer",
    (TiledSceneParser, "particle"): "a ParticleParser is out of scope for tiling (its rows are particles of an image, not images): bind "
                                    "a SceneParser, ParseRefiner, ParsePruner or ParseProposer",
    (SequenceTracker, "particle"): "a ParticleParser is out of scope for tiling (its rows are particles of an image, not images): bind "
                                   "a SceneParser, ParseRefiner, ParsePruner or ParseProposer"}


@pytest.mark.parametrize("cls", list(ACCEPTED), ids=lambda c: c.__name__)
def test_every_stage_binds_to_its_kinds_and_refuses_the_rest(cls):
    assert set(cls.ACCEPTS) == ACCEPTED[cls] <= set(stage.KINDS)
    for kind in stage.KINDS + (None,):
        provider = types.SimpleNamespace(KIND=kind, rows=lambda: {"what": kind}, what_sel=None, kept_step=None, kept_cand=None)
        if kind in ACCEPTED[cls]:
            assert cls.bind(provider) == {"what": kind}
            continue
        with pytest.raises(ValueError) as err:
            cls.bind(provider)
        if (cls, kind) in REFUSAL_TEXT:
            assert str(err.value) == REFUSAL_TEXT[(cls, kind)]
        with pytest.raises(ValueError):                            # the constructor refuses before it touches anything else
            cls(provider, *((1, 0.1, 0.1) if cls is ParseRefiner else (1,)))


def test_the_providers_say_what_they_are():
    from attend_infer_repeat_amd.parse import SceneParser
    from attend_infer_repeat_amd.particle_parse import ParticleParser
    from attend_infer_repeat_amd.trajectory import CompletedFrames
    kinds = {SceneParser: "scene", ParticleParser: "particle", ParseRefiner: "refiner", ParsePruner: "subset", ParseProposer: "subset",
             TemporalProposer: "subset", TiledSceneParser: "tiled", CompletedFrames: "completed"}
    for cls, kind in kinds.items():
        assert cls.KIND == kind and callable(cls.rows)
