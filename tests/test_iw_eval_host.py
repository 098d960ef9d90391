"""Host-only checks of the importance-weighted evaluation: the configuration refusal (pure Python) and the argument checks of
the two C-ABI entries, which return AIR_E_* before any launch (safe without a GPU)."""
import ctypes
import dataclasses

import pytest


@pytest.fixture(scope="module")
def lib():
    from attend_infer_repeat_amd import _lib, build
    build.build()
    return _lib.load()


def test_check_config_refuses_what_has_no_importance_weight():
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.iw_eval import check_config, inner_config
    cfg = EngineConfig()                                          # the training script's configuration
    assert check_config(cfg, 1) is None and check_config(cfg, 16) is None
    assert check_config(dataclasses.replace(cfg, where_shift_prior=(None, 1.0)), 4) is None      # a shift prior without loc is a density
    for bad, k, word in ((dict(discrete_steps=False), 4, "discrete_steps"), (dict(what_prior=None), 4, "what_prior"),
                         (dict(where_scale_prior=None), 4, "where_scale_prior"), (dict(where_shift_prior=None), 4, "where_shift_prior"),
                         ({}, 0, "particles"), ({}, -3, "particles")):
        with pytest.raises(ValueError, match=word):
            check_config(dataclasses.replace(cfg, **bad), k)
    # the training-loss extras do not enter: the inner engine drops them and keeps the model
    inner = inner_config(dataclasses.replace(cfg, l2_weight=1e-3, decay_rate=0.9, nsp_weight=3.0))
    assert inner.use_reinforce is False and inner.decay_rate is None and inner.l2_weight == 0.0
    assert inner.what_prior == cfg.what_prior and inner.max_steps == cfg.max_steps and inner.mfma_dtype == cfg.mfma_dtype


def test_evaluator_refuses_before_any_device_work():
    """the refusal comes from the host function: no engine is built, no HIP call is made"""
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.iw_eval import ImportanceEvaluator
    with pytest.raises(ValueError, match="discrete_steps"):
        ImportanceEvaluator(EngineConfig(discrete_steps=False), 4, 4, device="cpu")
    with pytest.raises(ValueError, match="particles"):
        ImportanceEvaluator(EngineConfig(), 4, 0, device="cpu")


def _ptr(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def test_iw_entries_report_argument_errors(lib):
    f = (ctypes.c_float * 64)()
    d = (ctypes.c_double * 8)()
    i = (ctypes.c_int * 16)()
    F, D, I = _ptr(f), _ptr(d), _ptr(i)
    pri = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)

    def logweight(T=3, R=8, K=4, A=2, **null):
        a = dict(what=F, what_loc=F, what_scale=F, where=F, where_loc=F, where_scale=F, presence=F, rec=F, logp=F, prior=D,
                 logw=F, n=I)
        a.update({k: None for k in null})
        return lib.air_iw_logweight(a["what"], a["what_loc"], a["what_scale"], a["where"], a["where_loc"], a["where_scale"],
                                    a["presence"], a["rec"], a["logp"], a["prior"], T, R, K, A, *pri, 1, a["logw"], a["n"], None)

    def reduce(T=3, R=8, K=4, gt=None, acc=None, **null):
        a = dict(logw=F, n=I, iw=F, elbo=F, ess=F, q=F)
        a.update({k: None for k in null})
        return lib.air_iw_reduce(a["logw"], a["n"], T, R, K, a["iw"], a["elbo"], a["ess"], a["q"], gt, acc, None)

    E_NULL, E_SHAPE = -1, -2
    for name in ("what", "what_scale", "where_loc", "presence", "rec", "logp", "prior", "logw", "n"):
        assert logweight(**{name: True}) == E_NULL, name
    for name in ("logw", "n", "iw", "elbo", "ess", "q"):
        assert reduce(**{name: True}) == E_NULL, name
    assert reduce(gt=I, acc=None) == E_NULL                       # counts need the totals block
    for fn in (logweight, reduce):
        assert fn(K=0) == E_SHAPE and fn(K=-2) == E_SHAPE
        assert fn(T=0) == E_SHAPE and fn(T=-1) == E_SHAPE and fn(T=33) == E_SHAPE
        assert fn(R=0) == E_SHAPE and fn(R=9, K=4) == E_SHAPE      # R is not a multiple of K
    assert logweight(A=0) == E_SHAPE
    assert lib.air_status_string(E_SHAPE).decode().startswith("AIR_E_SHAPE")
