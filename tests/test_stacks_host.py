"""stacks.py on the host: the normalised stack spec and its refusals, the one stack builder, the bounded cache, the sharing and drop
rules of the `parse` path of AIRonMNIST and the key of the track family -- against stub stages and a stub engine (no device)."""
import itertools
import types

import pytest

from attend_infer_repeat_amd import stacks
from attend_infer_repeat_amd.engine import EngineConfig
from attend_infer_repeat_amd.refine import DEFAULT_LR


class Stage:
    """a stage that remembers what it was built from and logs its life cycle"""

    def __init__(self, kind, log, provider, *args):
        self.kind, self.log, self.parser, self.args = kind, log, provider, args

    def capture(self):
        self.log.append(("capture", self))

    def release_graphs(self):
        self.log.append(("release", self))


def stub_classes(log):
    """stub constructors in the order of stacks.stage_classes()"""
    return tuple((lambda provider, *args, k=k: Stage(k, log, provider, *args)) for k in ("refine", "prune", "propose", "temporal"))


# ---- the spec ---------------------------------------------------------------------------------------------------------------------
def test_propose_and_temporal_spellings():
    for arg in ("propose", "temporal"):
        spec = lambda v: getattr(stacks.stack_spec(**{arg: v}), arg)
        assert spec(None) is None and spec(1) == (1, 1) and spec((1, 2)) == (1, 2) and spec([2, 2]) == (2, 2)
    for bad in ("one", (1, 2, 3), True):
        with pytest.raises(ValueError) as err:
            stacks.stack_spec(propose=bad)
        assert str(err.value) == "propose: the number of proposals per round, or (proposals, rounds), got %r" % (bad,)
        with pytest.raises(ValueError) as err:
            stacks.stack_spec(temporal=bad)
        assert str(err.value) == "temporal: the number of neighbour proposals per round, or (proposals, rounds), got %r" % (bad,)
    one, pair = stacks.stack_spec(propose=1), stacks.stack_spec(propose=(1, 1))
    assert one == pair and hash(one) == hash(pair) and {one: 0}[pair] == 0


def test_refine_and_its_learning_rates():
    assert stacks.stack_spec() == stacks.StackSpec(None, None, None, None, None)
    assert stacks.stack_spec(refine_lr=(1, 2, 3)).lr is None      # no refiner: nothing reads it
    spec = stacks.stack_spec(refine=2)
    assert spec.refine == 2 and spec.lr == tuple(float(v) for v in DEFAULT_LR) and len(spec.lr) == 2
    assert stacks.stack_spec(refine=2.0, refine_lr=[1, 0.5]) == stacks.stack_spec(refine=2, refine_lr=(1.0, 0.5))
    assert hash(stacks.stack_spec(refine=2.0, refine_lr=[1, 0.5])) == hash(stacks.stack_spec(refine=2, refine_lr=(1.0, 0.5)))
    for bad in ((0.1,), (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError) as err:
            stacks.stack_spec(refine=1, refine_lr=bad)
        assert str(err.value) == "refine_lr: (lr_what, lr_where), got %r" % (bad,)


def test_prune_together_with_propose_is_refused_under_every_name():
    texts = {"parse": "parse: prune together with propose is not supported: the search over the candidate pool already contains "
                      "prune=\"all\"; pass one of them",
             "parse_tiled": "parse_tiled: prune together with propose is not supported; pass one of them",
             "track": "track: prune together with propose is not supported; pass one of them",
             "temporal_proposer": "temporal_proposer: prune together with propose is not supported; pass one of them"}
    for who, text in texts.items():
        with pytest.raises(ValueError) as err:
            stacks.stack_spec(prune="all", propose=1, who=who)
        assert str(err.value) == text
    assert stacks.stack_spec(prune="all").prune == "all" and stacks.stack_spec(propose=1).prune is None


def test_require_engine_names_the_entry():
    eng = object()
    assert stacks.require_engine(types.SimpleNamespace(_engine=eng), "track") is eng
    for air in (types.SimpleNamespace(), types.SimpleNamespace(_engine=None)):
        with pytest.raises(NotImplementedError) as err:
            stacks.require_engine(air, "parse_tiled")
        assert str(err.value) == ("parse_tiled needs the fused engine: call train_step(...) with an engine-eligible configuration first "
                                  "(AIRonMNIST._engine is None on the generic autograd path)")


# ---- the builder ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine,subset,temporal", list(itertools.product((None, 3), (None, "prune", "propose"), (None, (2, 3)))))
def test_build_stack(refine, subset, temporal):
    log, base = [], object()
    spec = stacks.stack_spec(refine, (0.5, 0.25), "all" if subset == "prune" else None, (1, 2) if subset == "propose" else None, temporal)
    stack = stacks.build_stack(base, spec, n_frames=5, classes=stub_classes(log))
    want = [("refine", (3, 0.5, 0.25))] * (refine is not None) + [("prune", ("all",))] * (subset == "prune")
    want += [("propose", (1, 2))] * (subset == "propose") + [("temporal", (5, 2, 3))] * (temporal is not None)
    assert stack[0] is base and [(s.kind, s.args) for s in stack[1:]] == want
    assert all(s.parser is before for before, s in zip(stack, stack[1:]))          # each bound to its predecessor
    assert log == []                                                               # building captures nothing


def test_build_stack_takes_the_stage_classes_by_default():
    from attend_infer_repeat_amd.propose import ParseProposer
    from attend_infer_repeat_amd.prune import ParsePruner
    from attend_infer_repeat_amd.refine import ParseRefiner
    from attend_infer_repeat_amd.temporal import TemporalProposer
    assert stacks.stage_classes() == (ParseRefiner, ParsePruner, ParseProposer, TemporalProposer)


# ---- the cache --------------------------------------------------------------------------------------------------------------------
def test_cache_hit_miss_and_eviction_order():
    log, built = [], []
    cache = stacks.BoundedCache(lambda: 2)

    def build(name):
        def make():
            built.append(name)
            return stacks.captured([Stage(name + str(i), log, None) for i in range(3)])
        return make
    a = cache.get("a", build("a"))
    assert built == ["a"] and [e[0] for e in log] == ["capture"] * 3 and [e[1] for e in log] == a      # captured once, in stack order
    b = cache.get("b", build("b"))
    assert cache.get("a", build("a")) is a and built == ["a", "b"] and list(cache) == ["b", "a"]       # a hit: most recent now
    assert len(cache) == 2 and list(cache.values()) == [b, a] and list(cache.items()) == [("b", b), ("a", a)] and "a" in cache
    del log[:]
    c = cache.get("c", build("c"))                                 # over the limit: b is the least recently used
    assert list(cache) == ["a", "c"] and built == ["a", "b", "c"]
    assert [e for e in log if e[0] == "release"] == [("release", s) for s in reversed(b)]              # last member first, each once
    cache.limit = lambda: 1                                        # the limit is read when used
    assert cache.get("c", build("c")) is c and list(cache) == ["c"]
    assert [e[1] for e in log if e[0] == "release"] == list(reversed(b)) + list(reversed(a))


def test_cache_valid_and_drop_and_single_stages():
    log = []
    cache = stacks.BoundedCache(lambda: 4)
    make = lambda name: lambda: stacks.captured(Stage(name, log, None))
    one = cache.get("k", make("one"))
    assert cache.get("k", make("never"), valid=lambda e: e is one) is one
    two = cache.get("k", make("two"), valid=lambda e: False)      # found, but refused: released and rebuilt
    assert two is not one and two.kind == "two" and log[-2:] == [("release", one), ("capture", two)] and len(cache) == 1
    other = cache.get("o", make("other"))
    cache.drop(lambda e: e is two)
    assert list(cache.values()) == [other] and log[-1] == ("release", two)
    cache.drop(lambda e: False)
    assert list(cache) == ["o"] and log[-1] == ("release", two)

    def fails():
        raise ValueError("no")
    with pytest.raises(ValueError):
        cache.get("o", fails, valid=lambda e: False)
    assert len(cache) == 0 and log[-1] == ("release", other)       # a build that fails leaves no entry behind


def test_slot_rebuilds_when_the_identity_changed():
    log, owner = [], types.SimpleNamespace()
    first = stacks.slot(owner, "_held", lambda s: True, lambda: Stage("first", log, None))
    assert owner._held is first and log == [("capture", first)]
    assert stacks.slot(owner, "_held", lambda s: s is first, lambda: Stage("never", log, None)) is first and len(log) == 1
    second = stacks.slot(owner, "_held", lambda s: False, lambda: Stage("second", log, None))
    assert owner._held is second and log[1:] == [("release", first), ("capture", second)]


# ---- the `parse` path of the model ----------------------------------------------------------------------------------------------------
class Parser:
    def __init__(self, R, K=None, select=None):
        self.R = R
        if K is not None:
            self.K, self.select = K, select


@pytest.fixture
def air(monkeypatch):
    """an AIRonMNIST without its constructor: stub scene / particle parsers (rebuilt when the size changes, like the real holders)
    and stub stages behind them"""
    from attend_infer_repeat_amd.mnist_model import AIRonMNIST
    log = []
    monkeypatch.setattr(stacks, "stage_classes", lambda: stub_classes(log))
    air = AIRonMNIST.__new__(AIRonMNIST)
    air.log, air.obs, air._engine = log, types.SimpleNamespace(shape=(8, 50, 50)), "training-engine"

    def scene_parser(n):
        if getattr(air, "_scene_parser", None) is None or air._scene_parser.R != n:
            air._scene_parser = Parser(n)
        return air._scene_parser

    def particle_parser(n, K, select):
        s = getattr(air, "_particle_parser", None)
        if s is None or (s.R, s.K, s.select) != (n * K, K, select):
            air._particle_parser = Parser(n * K, K, select)
        return air._particle_parser
    air.scene_parser, air.particle_parser = scene_parser, particle_parser
    return air


def test_parse_path_shares_the_refiner_and_keys_as_before(air):
    plain = air._parser_for(2, "joint", 1, None)
    assert plain.kind == "refine" and plain.parser is air._particle_parser and plain.args == (1,) + tuple(DEFAULT_LR)
    pruned = air._parser_for(2, "joint", 1, None, "all")
    assert pruned.kind == "prune" and pruned.args == ("all",) and pruned.parser is plain and air._parser_for(2, "joint", 1, None) is plain
    proposed = air._parser_for(2, "joint", 1, None, None, 1)
    assert proposed.kind == "propose" and proposed.args == (1, 1) and proposed.parser is plain
    assert air._parser_for(2, "joint", 1, None, None, (1, 1)) is proposed and air._parser_for(2, "joint", 1, None, "all") is pruned
    assert list(air._parse_refiners) == [(16, 2, "joint", 1, tuple(DEFAULT_LR))]
    assert list(air._parse_pruners) == [(id(plain), "all")] and list(air._parse_proposers) == [(id(plain), 1, 1)]
    assert [e[0] for e in air.log] == ["capture"] * 3             # each built and captured once
    scene = air._parser_for(None, "joint")
    assert scene is air._scene_parser and air._parser_for(None, "joint", None, None, "present").parser is scene
    assert list(air._parse_pruners) == [(id(plain), "all"), (id(scene), "present")]
    with pytest.raises(ValueError, match="parse: prune together with propose is not supported: the search"):
        air._parser_for(None, "joint", None, None, "all", 1)
    with pytest.raises(ValueError, match="refine_lr"):
        air._parser_for(None, "joint", 1, (0.1,))


def test_parse_path_drops_what_a_rebuilt_parser_leaves_behind(air):
    refiner = air._parser_for(None, "joint", 2, None)
    pruner, proposer = air._parser_for(None, "joint", 2, None, "all"), air._parser_for(None, "joint", 2, None, None, 1)
    on_scene = air._parser_for(None, "joint", None, None, "all")
    assert len(air._parse_refiners) == 1 and len(air._parse_pruners) == 2 and len(air._parse_proposers) == 1
    air.obs = types.SimpleNamespace(shape=(4, 50, 50))             # another batch size: the scene parser is rebuilt
    del air.log[:]
    again = air._parser_for(None, "joint", 2, None, "all")
    assert again is not pruner and again.parser is not refiner and again.parser.parser is air._scene_parser
    assert list(air._parse_refiners.values()) == [again.parser] and list(air._parse_pruners.values()) == [again]
    released = [e[1] for e in air.log if e[0] == "release"]
    assert released == [refiner, pruner, on_scene]                 # the refiner on its lookup, its pruner and the old parser's next
    assert len(air._parse_proposers) == 1                          # the proposers are looked at on their next lookup
    assert air._parser_for(None, "joint", 2, None, None, 1) is not proposer and air.log[-2] == ("release", proposer)
    assert list(air._parse_proposers.values()) == [air._parser_for(None, "joint", 2, None, None, 1)]


def test_parse_path_rebuilds_an_entry_bound_to_another_provider(air):
    first = air._parser_for(None, "joint", 1, None)
    key = next(iter(air._parse_refiners))
    stale = Stage("refine", air.log, Parser(8))                    # under the same key, bound to another parser ...
    air._particle_parser = stale.parser                            # ... that is alive, so the drop rule leaves it
    air._parse_refiners[key] = stale
    second = air._parser_for(None, "joint", 1, None)
    assert second is not stale and second is not first and second.parser is air._scene_parser
    assert air.log[-2:] == [("release", stale), ("capture", second)] and list(air._parse_refiners.values()) == [second]


def test_parse_path_never_holds_more_than_the_limit(air):
    from attend_infer_repeat_amd.mnist_model import AIRonMNIST
    assert AIRonMNIST.MAX_PARSE_REFINERS == AIRonMNIST.MAX_PARSE_PRUNERS == AIRonMNIST.MAX_PARSE_PROPOSERS == 4
    assert AIRonMNIST.MAX_TILED_PARSERS == AIRonMNIST.MAX_TRACKERS == AIRonMNIST.MAX_TEMPORAL_PROPOSERS == 2
    for spec in (1, 2, 3, (2, 2), (3, 2), (1, 2)):
        air._parser_for(None, "joint", None, None, None, spec)
        assert len(air._parse_proposers) <= 4
    assert [k[1:] for k in air._parse_proposers] == [(3, 1), (2, 2), (3, 2), (1, 2)]
    for steps in range(1, 7):
        air._parser_for(None, "joint", steps, (0.1, 0.1), "present")
        assert len(air._parse_refiners) <= 4 and len(air._parse_pruners) <= 4
    assert [k[3] for k in air._parse_refiners] == [3, 4, 5, 6]
    air.MAX_PARSE_REFINERS = 1                                     # read when used
    air._parser_for(None, "joint", 6, (0.1, 0.1))
    assert [k[3] for k in air._parse_refiners] == [6]


# ---- the key of the track family ---------------------------------------------------------------------------------------------------
def test_track_key():
    eng = types.SimpleNamespace(cfg=EngineConfig(), device="cuda:0")
    S, F = 2, 3
    key = stacks.track_key(eng, S, F)
    assert key == stacks.track_key(eng, S, F, smooth=None, temporal=None, matching="greedy")
    assert hash(key) == hash(stacks.track_key(eng, S, F, smooth=None, temporal=None, matching="greedy"))
    from attend_infer_repeat_amd.track import DEFAULTS
    assert dict(key.assoc) == DEFAULTS and (key.S, key.F, key.smooth, key.matching, key.device) == (S, F, None, "greedy", "cuda:0")
    assert key.stack == stacks.stack_spec()
    others = [stacks.track_key(eng, S, F, **kw) for kw in (dict(smooth=True), dict(temporal=1), dict(matching="optimal"), dict(max_age=0),
                                                           dict(refine=1), dict(prune="all"), dict(propose=1))]
    assert len(set(others + [key])) == len(others) + 1
    assert key != stacks.track_key(types.SimpleNamespace(cfg=eng.cfg, device="cuda:1"), S, F) and key != stacks.track_key(eng, S, F + 1)
    assert stacks.track_key(eng, S, F, smooth=True) == stacks.track_key(eng, S, F, smooth=dict())
    assert stacks.track_key(eng, S, F, smooth=True) != stacks.track_key(eng, S, F, smooth=dict(horizon=2))
    assert stacks.track_key(eng, S, F, temporal=1, propose=1) == stacks.track_key(eng, S, F, temporal=(1, 1), propose=[1, 1])
    assert dict(stacks.track_key(eng, S, F, smooth=True).smooth)["horizon"] == 0


def test_track_key_checks_before_anything_is_built():
    eng = types.SimpleNamespace(cfg=EngineConfig(), device="cuda:0")
    with pytest.raises(ValueError, match="track: prune together with propose is not supported; pass one of them"):
        stacks.track_key(eng, 2, 3, prune="all", propose=1)
    with pytest.raises(ValueError, match="max_age must be an integer"):
        stacks.track_key(eng, 2, 3, max_age=1.5)
    with pytest.raises(ValueError, match="track: at least one sequence"):
        stacks.track_key(eng, 0, 3)
    with pytest.raises(ValueError, match="matching must be one of"):
        stacks.track_key(eng, 2, 3, matching="best")
    for bad in (0, (1, 0), (4, 1), "x", True):
        with pytest.raises(ValueError):
            stacks.track_key(eng, 2, 3, temporal=bad)
    with pytest.raises(ValueError, match="smooth"):
        stacks.track_key(eng, 2, 3, smooth=dict(unknown=1))


# ---- the stack behind a key of the track family -------------------------------------------------------------------------------------
def track_stub_classes(log):
    """stub constructors in the order of stacks.track_classes(); each remembers its keyword arguments too"""
    def make(kind):
        def build(provider, *args, **kwargs):
            stage = Stage(kind, log, provider, *args)
            stage.kwargs = kwargs
            return stage
        return build
    return tuple(make(k) for k in ("tracker", "stream_tracker", "smoother", "stream_smoother", "fitter"))


def test_track_classes_are_the_five_of_the_family():
    from attend_infer_repeat_amd import track, trajectory
    assert stacks.track_classes() == (track.SequenceTracker, track.StreamTracker, trajectory.TrajectorySmoother,
                                      trajectory.StreamSmoother, trajectory.TrajectoryNoiseFitter)


@pytest.mark.parametrize("kind", ["track", "track_smooth", "fit", "stream", "stream_smooth"])
def test_build_track_stack(kind):
    from attend_infer_repeat_amd.track import DEFAULTS, MOTION_GATE_DEFAULT, check_motion
    eng = types.SimpleNamespace(cfg=EngineConfig(), device="cuda:0")
    S, F, rule = 2, 5, dict(max_age=2, matching="optimal")
    moving = dict(motion=True, motion_gate=True)
    key = {"track": lambda: stacks.track_key(eng, S, F, **rule, **moving),
           "track_smooth": lambda: stacks.track_key(eng, S, F, smooth=dict(horizon=2), **rule, **moving),
           "fit": lambda: stacks.fit_key(eng, S, F, **rule, **moving),
           "stream": lambda: stacks.stream_key(eng, S, F, **rule),
           "stream_smooth": lambda: stacks.stream_smoother_key(eng, S, F, dict(lag=3), **rule)}[kind]()
    log, base = [], [object(), object()]
    stack = stacks.build_track_stack(list(base), key, classes=track_stub_classes(log))
    assert stack[:2] == base and log == []                         # behind the provider stack; building captures nothing
    tracker = stack[2]
    assert tracker.parser is base[-1] and tracker.args == (F,)     # bound to the last provider, over F frames
    want = dict(DEFAULTS, max_age=2, matching="optimal")
    if kind.startswith("stream"):
        assert tracker.kind == "stream_tracker" and tracker.kwargs == want          # no motion, no gate: not even as None
    else:
        assert tracker.kind == "tracker" and tracker.kwargs == dict(want, motion=check_motion(True), motion_gate=MOTION_GATE_DEFAULT)
    last = {"track": None, "track_smooth": "smoother", "fit": "fitter", "stream": None, "stream_smooth": "stream_smoother"}[kind]
    assert [s.kind for s in stack[3:]] == [last] * (last is not None)
    if last is not None:
        assert stack[3].parser is tracker                          # bound to the tracker
        if kind == "fit":
            assert stack[3].args == key.fit and stack[3].kwargs == {}
        else:
            assert stack[3].args == () and stack[3].kwargs == dict(key.smooth)
            assert stack[3].kwargs["horizon"] == (2 if kind == "track_smooth" else 0)
            assert ("lag" in stack[3].kwargs) == (kind != "track_smooth")
    plain = stacks.build_track_stack([base[0]], stacks.track_key(eng, S, F), classes=track_stub_classes(log))
    assert plain[1].kwargs == dict(DEFAULTS, matching="greedy", motion=None, motion_gate=None)


def test_the_stream_keys_take_no_smooth_among_the_trackers_arguments():
    eng = types.SimpleNamespace(cfg=EngineConfig(), device="cuda:0")
    with pytest.raises(TypeError, match="smooth"):
        stacks.stream_key(eng, 2, 5, smooth=True)
    with pytest.raises(TypeError, match="bogus"):
        stacks.stream_key(eng, 2, 5, bogus=1)
    with pytest.raises(TypeError, match="bogus"):
        stacks.track_key(eng, 2, 5, bogus=1)
