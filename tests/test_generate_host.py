"""Host-only checks of scene generation: the configuration refusal (pure Python), the two C-ABI entries in the header and the
ctypes table, and their argument checks, which return AIR_E_* before any launch (safe without a GPU)."""
import ctypes
import dataclasses
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from attend_infer_repeat_amd import _lib, build
    build.build()
    return _lib.load()


def test_check_config_refuses_what_defines_no_generative_density():
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.generate import check_config
    cfg = EngineConfig()                                          # the training script's configuration
    assert check_config(cfg) is None
    # neither the training-loss extras nor continuous steps enter the generative direction
    assert check_config(dataclasses.replace(cfg, discrete_steps=False, use_reinforce=False, l2_weight=1e-3)) is None
    for bad, word in ((dict(what_prior=None), "what_prior"), (dict(where_scale_prior=None), "where_scale_prior"),
                      (dict(where_shift_prior=None), "where_shift_prior"),
                      (dict(where_shift_prior=(None, 1.0)), r"where_shift_prior\[0\]")):
        with pytest.raises(ValueError, match=word):
            check_config(dataclasses.replace(cfg, **bad))
    with pytest.raises(ValueError, match="posterior's own mean"):
        check_config(dataclasses.replace(cfg, where_shift_prior=(None, 1.0)))


def test_sampler_refuses_before_any_device_work():
    """the refusal comes from the host function: no buffer is allocated, no HIP call is made"""
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.generate import SceneSampler
    with pytest.raises(ValueError, match="what_prior"):
        SceneSampler(EngineConfig(what_prior=None), 4, device="cpu")
    with pytest.raises(ValueError, match=r"where_shift_prior\[0\]"):
        SceneSampler(EngineConfig(where_shift_prior=(None, 1.0)), 4, device="cpu")
    with pytest.raises(ValueError, match="n_scenes"):
        SceneSampler(EngineConfig(), 0, device="cpu")


def test_count_table_of_caller_given_weights():
    from attend_infer_repeat_amd.generate import count_table
    assert count_table("uniform", 3) == [1.0, 1.0, 1.0, 1.0]
    assert count_table([0, 2, 0, 0.5], 3) == [0.0, 2.0, 0.0, 0.5]     # unnormalised weights, zeros allowed
    for bad in ("geometric", [1, 2, 3], [1, -1, 1, 1], [0, 0, 0, 0], [1, float("nan"), 1, 1], [1, float("inf"), 1, 1]):
        with pytest.raises(ValueError, match="count_probs"):
            count_table(bad, 3)


def test_header_and_ctypes_table_name_the_two_entries():
    from attend_infer_repeat_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "air_hip.h")).read(), flags=re.S)
    for name, n_args in (("air_prior_latents", 20), ("air_observe", 11)):
        m = re.search(r"AIR_ENGINE_API\s+int\s+%s\s*\(([^;]*)\);" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert "gen_kernels.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 10 and _lib.ENGINE_ABI_VERSION == 5


def _ptr(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def test_generate_entries_report_argument_errors(lib):
    f = (ctypes.c_float * 256)()
    d = (ctypes.c_double * 40)()
    i = (ctypes.c_int * 16)()
    s = (ctypes.c_uint64 * 2)()
    F, D, I, S = _ptr(f), _ptr(d), _ptr(i), _ptr(s)
    odd = ctypes.c_void_p(F.value + 4)                            # 4-byte aligned only
    pri = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)

    def latents(T=3, R=8, A=2, **over):
        a = dict(table=D, u=F, n_in=None, eps_what=F, eps_where=F, what=F, where=F, presence=F, n=I)
        a.update(over)
        return lib.air_prior_latents(a["table"], a["u"], a["n_in"], a["eps_what"], a["eps_where"], *pri, 0.0, T, R, A, a["what"],
                                     a["where"], a["presence"], a["n"], None)

    def observe(n=64, std=0.3, **over):
        a = dict(canvas=F, state=S, mean=F, obs=F)
        a.update(over)
        return lib.air_observe(a["canvas"], 0.5, std, a["state"], 0, float("nan"), float("nan"), a["mean"], a["obs"], n, None)

    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    for name in ("eps_what", "eps_where", "what", "where", "presence", "n"):
        assert latents(**{name: None}) == E_NULL, name
    assert latents(table=None) == E_NULL and latents(u=None) == E_NULL      # a drawn count needs both ...
    assert latents(table=None, u=None, n_in=I, R=0) == E_SHAPE              # ... a given one neither (the next check is reached)
    assert latents(T=0) == E_SHAPE and latents(T=-1) == E_SHAPE and latents(T=33) == E_SHAPE
    assert latents(R=0) == E_SHAPE and latents(R=-4) == E_SHAPE and latents(A=0) == E_SHAPE
    assert latents(where=odd) == E_ALIGN and latents(eps_where=odd) == E_ALIGN
    assert observe(canvas=None) == E_NULL and observe(mean=None, obs=None) == E_NULL
    assert observe(state=None) == E_NULL                          # noise needs the Philox state ...
    assert observe(state=None, std=0.0, n=0) == E_SHAPE           # ... std == 0 does not
    assert observe(n=0) == E_SHAPE
    assert lib.air_status_string(E_ALIGN).decode().startswith("AIR_E_ALIGN")
