"""Host-side checks of best-of-K scene parsing (attend_infer_repeat_amd/particle_parse.py, csrc/particle_kernels.hip): what the
constructor refuses, the argument errors of the three entries (returned before any launch: safe without a GPU), and how
AIRonMNIST.parse routes between the two parsers."""
import dataclasses

import pytest


def _cfg(**kw):
    from attend_infer_repeat_amd.engine_config import EngineConfig
    base = dict(what_prior=(0.0, 1.0), where_scale_prior=(0.0, 1.0), where_shift_prior=(0.0, 1.0))
    base.update(kw)
    return EngineConfig(**base)


def test_check_arguments_refusals():
    from attend_infer_repeat_amd.particle_parse import CRITERIA, ParticleParser, check_arguments
    cfg = _cfg()
    check_arguments(cfg, 4, 16, "joint")
    check_arguments(cfg, 1, 1, "weight")
    assert CRITERIA == {"weight": 0, "joint": 1}
    with pytest.raises(ValueError, match="particles >= 1"):
        check_arguments(cfg, 4, 0, "joint")
    with pytest.raises(ValueError, match="select"):
        check_arguments(cfg, 4, 4, "map")
    with pytest.raises(ValueError, match="batch_size >= 1"):
        check_arguments(cfg, 0, 4, "joint")
    with pytest.raises(ValueError, match="what_prior"):
        check_arguments(dataclasses.replace(cfg, what_prior=None), 4, 4, "joint")
    with pytest.raises(ValueError, match="where_scale_prior"):
        check_arguments(dataclasses.replace(cfg, where_shift_prior=None), 4, 4, "joint")
    with pytest.raises(ValueError, match="discrete_steps"):
        check_arguments(dataclasses.replace(cfg, discrete_steps=False), 4, 4, "joint")
    # the constructor runs the same checks before it touches a device
    for args, kw, pat in (((cfg, 4, 0), {}, "particles >= 1"), ((cfg, 4, 4), {"select": "best"}, "select"),
                          ((cfg, 0, 4), {}, "batch_size >= 1")):
        with pytest.raises(ValueError, match=pat):
            ParticleParser(*args, **kw)


@pytest.fixture(scope="module")
def lib():
    from attend_infer_repeat_amd import _lib, build
    build.build()
    return _lib.load()


X = 4096          # a non-NULL, 16-byte aligned stand-in: the entries return before they would dereference it
NULL, SHAPE = -1, -2


def _logposterior(lib, T=3, R=8, K=4, A=5, out=X, what=X):
    return lib.air_iw_logposterior(what, X, X, X, X, X, X, X, T, R, K, A, out, None)


def _select(lib, T=3, R=8, K=4, A=5, G=6, criterion=1, log_q=X, outs=(X,) * 8):
    return lib.air_particle_select(X, log_q, X, X, X, X, X, T, R, K, A, G, criterion, *outs, None)


def _spread(lib, T=3, R=8, K=4, outs=(X, X, X)):
    return lib.air_particle_spread(X, X, X, T, R, K, *outs, None)


def test_entries_report_argument_errors_without_launching(lib):
    """NULL / bad-shape arguments return AIR_E_* before any launch (the style of test_argument_errors_are_reported_not_crashed)"""
    for call in (_logposterior, _select, _spread):
        assert call(lib, K=0) == SHAPE, call.__name__
        assert call(lib, T=33) == SHAPE, call.__name__
        assert call(lib, T=0) == SHAPE, call.__name__
        assert call(lib, R=9, K=4) == SHAPE, call.__name__               # R % K != 0
    assert _logposterior(lib, out=None) == NULL and _logposterior(lib, what=None) == NULL
    assert _logposterior(lib, A=0) == SHAPE
    for i in range(8):                                                   # every output of the select entry
        outs = [X] * 8
        outs[i] = None
        assert _select(lib, outs=tuple(outs)) == NULL, i
    assert _select(lib, criterion=1, log_q=None) == NULL                 # "joint" needs log q; "weight" does not read it
    assert _select(lib, criterion=2) == SHAPE and _select(lib, G=0) == SHAPE
    for i in range(3):
        outs = [X] * 3
        outs[i] = None
        assert _spread(lib, outs=tuple(outs)) == NULL, i


class _StubParser:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def load_from(self, engine):
        self.log.append((self.name, "load_from", engine))

    def parse(self, *args):
        self.log.append((self.name, "parse") + args)
        return {"parser": self.name}


def _stub_model():
    from attend_infer_repeat_amd.mnist_model import AIRonMNIST
    air = AIRonMNIST.__new__(AIRonMNIST)
    log = []
    air.obs = type("Obs", (), {"shape": (8, 50, 50)})()
    air._engine = "training-engine"
    air._sync_engine_switches = lambda: log.append(("sync",))
    air.scene_parser = lambda n: log.append(("scene_parser", n)) or _StubParser(log, "scene")
    air.particle_parser = lambda n, k, sel: log.append(("particle_parser", n, k, sel)) or _StubParser(log, "particle")
    return air, log


def test_parse_without_particles_takes_the_scene_parser():
    air, log = _stub_model()
    assert air.parse() == {"parser": "scene"} and air.parsed == {"parser": "scene"}
    assert log == [("scene_parser", 8), ("sync",), ("scene", "load_from", "training-engine"), ("scene", "parse", air.obs, None)]
    del log[:]
    air.parse(num_objects=2)
    assert log[0] == ("scene_parser", 8) and log[-1] == ("scene", "parse", air.obs, 2)
    assert not any(e[0] == "particle_parser" for e in log)


def test_parse_with_particles_takes_the_particle_parser():
    air, log = _stub_model()
    assert air.parse(particles=4) == {"parser": "particle"}
    assert log == [("particle_parser", 8, 4, "joint"), ("sync",), ("particle", "load_from", "training-engine"),
                   ("particle", "parse", air.obs)]
    del log[:]
    air.parse(particles=16, select="weight")
    assert log[0] == ("particle_parser", 8, 16, "weight")


def test_counts_and_particles_together_are_refused():
    air, log = _stub_model()
    with pytest.raises(ValueError, match="num_objects together with particles"):
        air.parse(num_objects=2, particles=4)
    assert log == []
