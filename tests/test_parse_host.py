"""Host-only checks of scene parsing: the configuration refusal (pure Python), the two C-ABI entries in the header and the ctypes
table, and their argument checks, which return AIR_E_* before any launch (safe without a GPU)."""
import ctypes
import dataclasses
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from attend_infer_repeat_amd import _lib, build
    build.build()
    return _lib.load()


def test_check_config_refuses_continuous_steps_only():
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import check_config
    cfg = EngineConfig()                                          # the training script's configuration
    assert check_config(cfg) is None
    # no prior enters the parse; the training-loss extras do not either
    assert check_config(dataclasses.replace(cfg, what_prior=None, where_scale_prior=None, where_shift_prior=None,
                                            use_reinforce=False, l2_weight=1e-3, nsp_analytic=False)) is None
    with pytest.raises(ValueError, match="discrete_steps"):
        check_config(dataclasses.replace(cfg, discrete_steps=False))


def test_parser_refuses_before_any_device_work():
    """the refusals come from host code: no buffer is allocated, no HIP call is made"""
    from attend_infer_repeat_amd import _lib
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    with pytest.raises(ValueError, match="discrete_steps"):
        SceneParser(EngineConfig(discrete_steps=False), 4, device="cpu")
    with pytest.raises(ValueError, match="batch_size"):
        SceneParser(EngineConfig(), 0, device="cpu")
    with pytest.raises(_lib.AirHipError, match="no CPU fallback"):
        SceneParser(EngineConfig(), 4, device="cpu")


def test_header_and_ctypes_table_name_the_two_entries():
    from attend_infer_repeat_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "air_hip.h")).read(), flags=re.S)
    for name, n_args in (("air_parse_objects", 22), ("air_parse_render", 20)):
        m = re.search(r"AIR_ENGINE_API\s+int\s+%s\s*\(([^;]*)\);" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert "parse_kernels.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 10 and _lib.ENGINE_ABI_VERSION == 5
    assert re.search(r"#define\s+AIR_ABI_VERSION\s+10\b", src) and re.search(r"#define\s+AIR_ENGINE_ABI_VERSION\s+5\b", src)


def _ptr(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


OBJ_OUT = ("num_objects", "count_prob", "presence", "score", "boxes", "offsets", "obj_image", "obj_step", "obj_box", "obj_score",
           "obj_where", "obj_what")


def test_parse_objects_reports_argument_errors(lib):
    f = (ctypes.c_float * 256)()
    i = (ctypes.c_int * 64)()
    F, I = _ptr(f), _ptr(i)
    odd = ctypes.c_void_p(F.value + 4)                            # 4-byte aligned only

    def objects(T=3, R=4, A=2, H=8, W=8, **over):
        a = dict(prob=F, n_in=None, where=F, what=F, num_objects=I, count_prob=F, presence=F, score=F, boxes=F, offsets=I,
                 obj_image=I, obj_step=I, obj_box=F, obj_score=F, obj_where=F, obj_what=F)
        a.update(over)
        return lib.air_parse_objects(a["prob"], a["n_in"], a["where"], a["what"], T, R, A, H, W, *[a[k] for k in OBJ_OUT], None)

    for name in ("where", "what") + OBJ_OUT:
        assert objects(**{name: None}) == E_NULL, name
    assert objects(prob=None) == E_NULL                           # the model's count needs the probabilities ...
    assert objects(prob=None, n_in=I, R=0) == E_SHAPE             # ... a given one does not (the next check is reached)
    assert objects(T=0) == E_SHAPE and objects(T=33) == E_SHAPE
    assert objects(R=0) == E_SHAPE and objects(R=-4) == E_SHAPE
    assert objects(A=0) == E_SHAPE and objects(A=-1) == E_SHAPE
    assert objects(H=0) == E_SHAPE and objects(W=0) == E_SHAPE
    for name in ("where", "boxes", "obj_box", "obj_where"):
        assert objects(**{name: odd}) == E_ALIGN, name


def test_parse_render_reports_argument_errors(lib):
    f = (ctypes.c_float * 256)()
    i = (ctypes.c_int * 64)()
    b = (ctypes.c_byte * 64)()
    F, I, B8 = _ptr(f), _ptr(i), _ptr(b)
    odd = ctypes.c_void_p(F.value + 4)

    def render(T=3, R=2, H=4, W=4, h=2, w=2, n_bands=1, **over):
        a = dict(glimpse=F, where=F, presence=F, obs=F, reconstruction=F, rec_parts=F, owner=B8, area=I, layers=None)
        a.update(over)
        return lib.air_parse_render(a["glimpse"], a["where"], a["presence"], a["obs"], 0.5, 0.3, 0.02, T, R, H, W, h, w, n_bands,
                                    a["reconstruction"], a["rec_parts"], a["owner"], a["area"], a["layers"], None)

    for name in ("glimpse", "where", "presence", "reconstruction", "owner", "area"):
        assert render(**{name: None}) == E_NULL, name
    assert render(obs=None) == E_NULL                             # the reconstruction term needs the observation ...
    assert render(obs=None, rec_parts=None, R=0) == E_SHAPE       # ... without it none is wanted (the next check is reached)
    assert render(T=0) == E_SHAPE and render(T=33) == E_SHAPE
    assert render(R=0) == E_SHAPE and render(R=-1) == E_SHAPE
    for dim in ("H", "W", "h", "w", "n_bands"):
        assert render(**{dim: 0}) == E_SHAPE, dim
    assert render(n_bands=3) == E_SHAPE                           # 4 rows in 3 bands of 2 rows are 2 bands: rec_parts would be mis-sized
    assert render(where=odd) == E_ALIGN
    assert lib.air_status_string(E_ALIGN).decode().startswith("AIR_E_ALIGN")
