"""GPU parity of the fused launches around the glimpse read and of the `what` head, one kernel at a time (run with -m gpu on an MI355X):
air_attend_fwd, air_attend_bwd, air_attend_bwd_dx, air_what_head_fwd, air_what_sample_pack against the float64 references of
tests/attend_cases.py, where every case is listed with the launch path it reaches (tests/test_attend_cases_host.py checks the list
against the selection rules on the CPU).

Group letters continue those of tests/test_objective_kernels.py: D attend forward, E attend backward, F `what` head; the worst
error / tolerance ratio of each group is printed when the module finishes (pytest -s).  Every output buffer starts as NaN (the
wrappers of attend_infer_repeat_amd/hip.py), so an element a launch leaves out fails the comparison it belongs to."""
import numpy as np
import pytest
import torch

import attend_cases as AC
from attend_cases import assert_bits, assert_close, g
from oracle import st_loops as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu_device):
    from attend_infer_repeat_amd import hip as H
    H.lib()
    return H


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    AC.print_worst("attend kernels", "DEF")


def _no_nan(tag, **tensors):
    for nm, t in tensors.items():
        assert not bool(torch.isnan(t).any()), f"{tag}{nm}: {int(torch.isnan(t).sum())} of {t.numel()} elements were not written"


def _ids(cases):
    return [f"{i}-T{c[0]}-B{c[1]}" for i, c in enumerate(cases)]


# ---------------------------------------------------------------------------------------------------------------
# D. air_attend_fwd
# ---------------------------------------------------------------------------------------------------------------
def _attend_fwd(hip, c, **replace):
    t = {k: g(c[k]) for k in ("tr_h", "tr_w", "tr_b", "st_h", "st_w", "st_b", "eps", "u", "img")}
    t.update(replace)
    return hip.attend_fwd(t["tr_h"], t["tr_w"], t["tr_b"], t["st_h"], t["st_w"], t["st_b"], t["eps"], AC.RAW_OFFSET, AC.PRIOR4, t["u"],
                          c["step_bias"], c["explore_eps"], c["prior"].cuda(), t["img"], (c["h"], c["w"]), c["precision"], c["guard_eps"])


@pytest.mark.parametrize("i", range(len(AC.FWD_CASES)), ids=_ids(AC.FWD_CASES))
def test_attend_fwd(hip, i):
    c = AC.fwd_case(i)
    T, B, h, w = c["T"], c["B"], c["h"], c["w"]
    tag = f"attend_fwd case {i} {AC.FWD_CASES[i]} "
    (pre, logit), (loc, scale, where, kl_row), count, glimpse = _attend_fwd(hip, c)
    _no_nan(tag, pre=pre, logit=logit, loc=loc, scale=scale, where=where, kl_row=kl_row, glimpse=glimpse,
            **dict(zip(("prob", "presence", "q", "kl", "logp", "step_weight"), count)))
    # the two output layers: the forward tolerance of test_linear_fwd_bwd
    assert_close(pre, c["pre64"], 2e-5, 2e-5, tag + "pre", "D"); assert_close(logit, c["logit64"], 2e-5, 2e-5, tag + "logit", "D")
    # the where head: the tolerances of test_gauss_sample_fwd_bwd
    assert_close(loc, c["loc64"], 1e-5, 1e-6, tag + "loc", "D"); assert_close(scale, c["scale64"], 1e-5, 1e-6, tag + "scale", "D")
    assert_close(where, c["where64"], 1e-5, 1e-5, tag + "where", "D"); assert_close(kl_row, c["kl_row64"], 1e-5, 1e-4, tag + "kl_row", "D")
    if c["guard_eps"] > 0:
        assert float(scale[0, 0]) == np.float32(c["guard_eps"]) and int((scale <= c["guard_eps"]).sum()) == 1
    # the count side: no presence draw can flip (the p of the kernel's logit stays within a tenth of the margin of u), then exactly
    p_kernel = AC._presence_prob64(logit.cpu().double(), c["step_bias"], c["explore_eps"])
    assert float((p_kernel - c["p64"]).abs().max()) < AC.U_MARGIN / 10
    AC._check_fused_forward(count, c, c["prior"], tag, "D")
    # the glimpses: the bits of the oracle's read at the `where` the launch wrote
    ref = C.st_read_fwd(np.tile(c["img"].numpy(), (T, 1, 1)), where.cpu().numpy(), (h, w))
    np.testing.assert_array_equal(glimpse.cpu().numpy(), ref, err_msg=tag + "glimpse")


def test_attend_fwd_declines_what_it_cannot_stage(hip):
    """H*W % 4 != 0, an img or a tr_w that is not 16-byte aligned: AIR_E_UNSUPPORTED (-5) from the argument checks, before any launch
    (every pointer handed over is valid memory of the full size)"""
    from attend_infer_repeat_amd._lib import AirHipError
    T, B, H, W, h, w, tr_k, st_k = AC.FWD_UNSUPPORTED
    c = AC.attend_inputs(4999, T, B, H, W, h, w, tr_k, st_k, AC.F32, False, 0.0, None)
    with pytest.raises(AirHipError, match="status -5"):
        _attend_fwd(hip, c)
    c = AC.fwd_case(0)

    def offset_view(t):                                                         # the same values, 4 bytes into a larger buffer
        buf = torch.zeros(t.numel() + 8, device="cuda")
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    for name in ("img", "tr_w"):
        with pytest.raises(AirHipError, match="status -5"):
            _attend_fwd(hip, c, **{name: offset_view(c[name])})
    torch.cuda.synchronize()
    _attend_fwd(hip, c)                                                         # and the aligned launch goes through
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# E. air_attend_bwd, air_attend_bwd_dx
# ---------------------------------------------------------------------------------------------------------------
def _padded(values, ld, pad):
    """values[M, k] as a row view of a [M, ld] buffer whose other columns hold `pad`"""
    M, k = values.shape
    buf = torch.full((M, ld), pad, dtype=torch.float32, device="cuda")
    buf[:, :k] = values.cuda()
    return buf, buf[:, :k]


@pytest.mark.parametrize("i", range(len(AC.BWD_CASES)), ids=_ids(AC.BWD_CASES))
def test_attend_bwd_and_its_dx_form(hip, i):
    c = AC.bwd_case(i)
    T, B, H, W, M = c["T"], c["B"], c["H"], c["W"], c["T"] * c["B"]
    tag = f"attend_bwd case {i} [{c['name']}] "
    args = (g(c["img"]), g(c["where"]), g(c["dglimpse"]), g(c["pre"]), g(c["eps"]), AC.RAW_OFFSET, AC.PRIOR4, g(c["loc"]), g(c["scale"]),
            g(c["dwhere_w"]), g(c["dkl_row"]), AC.DKL_SCALE, g(c["prob"]), g(c["presence"]), c["prior"].cuda(), AC.KL_SCALE, g(c["ka"]),
            g(c["kb"]), AC.W_SCALE, g(c["dlogp"]), g(c["dpres"]), g(c["logit"]), c["step_bias"], c["explore_eps"])
    plain = hip.attend_bwd(*args)
    # the _dx form: activations and outputs as row views of [M, ld] buffers; the padding of the activations is NaN (a read at the wrong
    # leading dimension poisons its output), the padding of the outputs a sentinel that must survive
    nan = float("nan")
    tr_buf, tr_dx = _padded(torch.full((M, c["tr_k"]), nan), c["tr_ld"], AC.SENTINEL)
    st_buf, st_dx = _padded(torch.full((M, c["st_k"]), nan), c["st_ld"], AC.SENTINEL)
    tr_y = _padded(c["tr_y"], c["tr_ld"], nan)[1] if c["tr_y"] is not None else None
    st_y = _padded(c["st_y"], c["st_ld"], nan)[1] if c["st_y"] is not None else None
    fused = hip.attend_bwd(*args, tr_w=g(c["tr_w"]), tr_y=tr_y, tr_dx=tr_dx, st_w=g(c["st_w"]), st_y=st_y, st_dx=st_dx,
                           precision=c["precision"])
    assert fused[3] is tr_dx and fused[4] is st_dx
    norm = (c["dglimpse"].abs().sum((1, 2))[:, None] * max(H, W) / 2 * 0.05 + 1.0).double()      # the normalisation of test_st_read_bwd
    for form, (dwhere_r, dpre, dlogit) in (("air_attend_bwd ", plain), ("air_attend_bwd_dx ", fused[:3])):
        _no_nan(tag + form, dwhere_r=dwhere_r, dpre=dpre, dlogit=dlogit)
        assert_close(dwhere_r.cpu().double() / norm, c["dwhere_r64"] / norm, 1e-4, 2e-5, tag + form + "dwhere_r", "E")
        # d pre: the float64 chain at the d where the kernel itself read back (the conditioning of the read is judged once, above)
        assert_close(dpre, AC.dpre_ref(c, dwhere_r.cpu()), 1e-4, 1e-5, tag + form + "dpre", "E")
        assert_close(dlogit, c["dlogit64"], 2e-4, 2e-4, tag + form + "dlogit", "E")
    for a, b, nm in zip(plain, fused, ("dwhere_r", "dpre", "dlogit")):
        assert_bits(a, b, tag + nm + " of air_attend_bwd against air_attend_bwd_dx")
    # the two dX products on the d pre / d logit the launch wrote (operands rounded to bf16 for precision 1): the dx tolerance of
    # test_linear_fwd_bwd
    _no_nan(tag, tr_dx=tr_dx, st_dx=st_dx)
    tr_ref, st_ref = AC.dx_ref(c, fused[1], fused[2], c["precision"])
    assert_close(tr_dx, tr_ref, 1e-4, 1e-4, tag + "tr_dx", "E"); assert_close(st_dx, st_ref, 1e-4, 1e-4, tag + "st_dx", "E")
    for buf, k, nm in ((tr_buf, c["tr_k"], "tr_dx"), (st_buf, c["st_k"], "st_dx")):
        assert_bits(buf[:, k:], torch.full_like(buf[:, k:], AC.SENTINEL), tag + nm + " padding columns")


# ---------------------------------------------------------------------------------------------------------------
# F. air_what_head_fwd, air_what_sample_pack
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(AC.WHAT_CASES)), ids=_ids(AC.WHAT_CASES))
def test_what_head_and_sample_pack(hip, i):
    c = AC.what_case(i)
    T, B, K, A, M = c["T"], c["B"], c["K"], c["A"], c["T"] * c["B"]
    tag = f"what_head case {i} {AC.WHAT_CASES[i]} "
    if c["offset"]:                                                             # 4 bytes into its buffer: the scalar loads
        buf = torch.zeros(M * c["ldx"] + 8, device="cuda")
        xb = buf[1:1 + M * c["ldx"]].view(M, c["ldx"])
        xb.copy_(c["x_buf"])
        assert xb.data_ptr() % 16 == 4
    else:
        xb = g(c["x_buf"])
    x = xb[:, :K]
    eps, where, presence, states = g(c["eps"]), g(c["where"]), g(c["presence"]), [g(s) for s in c["states"]]
    q, loc, scale, sample, kl_parts, pack = hip.what_head_fwd(x, g(c["w"]), g(c["b"]), eps, AC.WHAT_OFFSET, AC.WHAT_PRIOR, where, presence,
                                                              states, T, c["precision"])
    assert kl_parts.shape == ((A + 7) // 8, M)                                  # no rows beyond M exist
    _no_nan(tag, q=q, loc=loc, scale=scale, sample=sample, kl_parts=kl_parts, pack=pack)
    assert_close(q, c["q64"], 2e-5, 2e-5, tag + "q", "F")                      # the forward tolerance of test_linear_fwd_bwd
    assert_bits(loc, q[:, :A].contiguous(), tag + "loc = the first half of q")
    assert_close(loc, c["loc64"], 1e-5, 1e-6, tag + "loc", "F"); assert_close(scale, c["scale64"], 1e-5, 1e-6, tag + "scale", "F")
    assert_close(sample, c["sample64"], 1e-5, 1e-5, tag + "sample", "F")
    # every column of pack_out: an indexed copy of what the launch wrote and was given
    assert_bits(pack, AC.pack_ref(sample.cpu(), c["where"], c["presence"], c["states"], T, B), tag + "pack_out")
    kl = kl_parts[0].cpu().clone()
    for part in range(1, kl_parts.shape[0]):
        kl = kl + kl_parts[part].cpu()                                          # float32, in tile order, as the consumer adds them
    assert_close(kl, c["kl_row64"], 1e-5, 1e-4, tag + "sum of kl_parts", "F")
    # air_what_sample_pack on the q the head wrote: the bits of the head
    loc2, scale2, sample2, kl_row2, pack2 = hip.what_sample_pack(q, eps, AC.WHAT_OFFSET, AC.WHAT_PRIOR, where, presence, states, T)
    _no_nan(tag + "what_sample_pack ", loc=loc2, scale=scale2, sample=sample2, kl_row=kl_row2, pack=pack2)
    for a, b, nm in ((loc2, loc, "loc"), (scale2, scale, "scale"), (sample2, sample, "sample"), (pack2, pack, "pack_out")):
        assert_bits(a, b, tag + nm + " of air_what_sample_pack against air_what_head_fwd")
    assert_close(kl_row2, c["kl_row64"], 1e-5, 1e-4, tag + "kl_row of air_what_sample_pack", "F")
