"""The cases of tests/test_attend_kernels.py on the CPU: every case builds (its conditions are asserted where its inputs are made,
tests/attend_cases.py), every case reaches the launch path its comment names (the selection rules of csrc/st_kernels.hip restated
here), and the float64 references agree with independent ones: d where through the read with autograd through the oracle's read,
d pre with central finite differences of the float64 forward."""
import pytest
import torch

import attend_cases as AC
from oracle import air_oracle as O


@pytest.mark.parametrize("i", range(len(AC.FWD_CASES)))
def test_forward_case_builds_with_its_conditions(i):
    c = AC.fwd_case(i)
    T, B = c["T"], c["B"]
    assert c["pre64"].shape == (T * B, 8) and c["logit64"].shape == (T, B) and c["where64"].shape == (T * B, 4)
    if c["u"] is not None:
        assert bool(((c["u"].double() - c["p64"]).abs() >= AC.U_MARGIN).all())
        assert set(c["pres"].unique().tolist()) <= {0.0, 1.0}
    else:
        frac = torch.remainder(c["p64"].sum(0), 1.0)
        assert bool(((frac >= 0.05) & (frac <= 0.95)).all())
    assert bool((c["count"] >= 0).all()) and bool((c["count"] <= T).all())
    # every glimpse overlaps its image: the oracle's read of an image of ones at the reference's where
    glimpse = O.st_read(torch.ones(T * B, c["H"], c["W"], dtype=torch.float64), c["where64"], (c["h"], c["w"]))
    assert bool((glimpse.reshape(T * B, -1).abs().sum(1) > 0).all())


def _fwd_path(T, B, H, W, h, w):
    """launch selection of air_attend_fwd: (threads, template, image-major, lean)"""
    nq = H * W // 4
    img_major = T * B > 2048 and T > 1
    lean = img_major and w % 4 == 0 and W >= 4
    threads = 256 if nq <= 768 else 512 if (nq <= 2560 and not img_major and T * B > 256) else 1024
    mt = "3" if T == 3 else "5" if T == 5 else "8" if T <= 8 else "32"
    return threads, mt, img_major, lean


def test_forward_cases_reach_every_launch_path():
    paths = [_fwd_path(*case[:6]) for case in AC.FWD_CASES]
    assert {p[0] for p in paths} == {256, 512, 1024}
    assert {p[1] for p in paths} == {"3", "5", "8", "32"}
    assert {(p[2], p[3]) for p in paths} == {(False, False), (True, False), (True, True)}
    major = [(case, p) for case, p in zip(AC.FWD_CASES, paths) if p[2]]
    waves = lambda p: p[0] // 64
    assert any(case[0] > waves(p) and p[3] for case, p in major) and any(case[0] < waves(p) and p[3] for case, p in major)
    assert any(case[0] > waves(p) and not p[3] for case, p in major)
    assert {"8", "32"} <= {p[1] for _, p in major}
    assert any(case[5] % 4 == 0 and case[3] < 4 and not p[3] for case, p in major)          # W < 4 keeps the per-pixel form
    assert any(c[6] < 64 for c in AC.FWD_CASES) and any(c[6] % 64 for c in AC.FWD_CASES if c[6] > 64)
    assert any(c[7] < 4 for c in AC.FWD_CASES) and any(c[7] % 16 == 0 for c in AC.FWD_CASES) and any(c[7] % 4 for c in AC.FWD_CASES)
    assert {c[8] for c in AC.FWD_CASES} == {AC.F32, AC.BF16} and {c[9] for c in AC.FWD_CASES} == {True, False}
    assert sum(1 for c in AC.FWD_CASES if c[12] > 0) == 1
    T, B, H, W = AC.FWD_UNSUPPORTED[:4]
    assert (H * W) % 4 != 0


@pytest.mark.parametrize("i", range(len(AC.BWD_CASES)))
def test_backward_case_builds_with_its_conditions(i):
    c = AC.bwd_case(i)
    M = c["T"] * c["B"]
    assert c["dwhere_r64"].shape == (M, 4) and c["dpre64"].shape == (M, 8) and c["dlogit64"].shape == (c["T"], c["B"])
    for k in ("tr_y", "st_y"):
        if c[k] is not None:
            assert bool((c[k].abs() >= 1e-3).all())
    wh = c["where"]
    assert bool(((wh[:, 0::2] >= 0.2 - 1e-4) & (wh[:, 0::2] <= 1.4 + 1e-4) & (wh[:, 1::2].abs() <= 0.8 + 1e-4)).all())
    assert bool((c["dwhere_r64"].abs().sum(1) > 0).all())                       # every glimpse overlaps its image
    assert c["tr_ld"] >= c["tr_k"] and c["st_ld"] >= c["st_k"]


def _bwd_path(T, B, H, W, h, w):
    """launch selection of attend_bwd_launch: (threads, template, image-major, fast form, vec4)"""
    img_major = T * B > 2048 and T > 1
    hw = h * w
    threads = 256 if (hw <= 256 or (img_major and hw <= 1024)) else 512 if hw <= 512 else 1024
    fast = img_major and T * (threads // 64 * 8 + 8) <= 3 * w + 3 * h + 160
    mt = "3" if T == 3 else "5" if T == 5 else "8" if T <= 8 else "32"
    return threads, mt, img_major, fast, (H * W) % 4 == 0


def test_backward_cases_reach_every_launch_path():
    cases = AC.BWD_CASES
    paths = [_bwd_path(*case[:6]) for case in cases]
    assert {p[0] for p in paths if not p[2]} == {256, 512, 1024}
    assert {p[1] for p in paths} == {"3", "5", "8", "32"}
    assert any(p[2] and p[3] and p[0] == 256 for p in paths) and any(p[2] and p[3] and p[0] == 1024 for p in paths)
    assert {p[1] for p in paths if p[2] and not p[3]} >= {"5", "32"}            # the per-glimpse loop, image-major
    assert any(not p[4] for p in paths)                                         # vec4 = 0
    assert {case[6] for case in cases} == {(40, 40), (256, 260), (600, 604)}
    assert {case[7] for case in cases} == {(1, 1), (50, 53), (130, 130)}
    assert {case[10] for case in cases} == {1, 2, 3, 4}
    assert {case[8] for case in cases} == {True, False} and {case[9] for case in cases} == {True, False}
    assert {AC.BWD_VARIANTS[case[11]][1] for case in cases} == {True, False}
    assert sum(1 for case in cases if not case[12]) == 1 and sum(1 for case in cases if case[13] == AC.BF16) == 2
    # the second pass of the fused transform dX (n0 != tid) with tr_y at tr_ld > tr_k: outside the fast form, tr_k > 2 * threads
    assert any(case[6][0] > 2 * p[0] and case[6][1] > case[6][0] and case[8] and not p[3] for case, p in zip(cases, paths))
    # role B of the _dx form past its first 4 * threads outputs
    assert any(16 * case[0] * case[7][0] > 4 * p[0] for case, p in zip(cases, paths))
    assert any(case[1] % 16 for case in cases) and any(case[1] > 64 for case in cases)
    # slabs beyond the first inside the fast form and outside it
    assert any(case[10] > 1 and p[3] for case, p in zip(cases, paths)) and any(case[10] > 1 and not p[3] for case, p in zip(cases, paths))


@pytest.mark.parametrize("i", [0, 4])
def test_backward_reference_of_the_read_equals_autograd_through_the_oracle_read(i):
    c = AC.bwd_case(i)
    where = c["where"].double().requires_grad_(True)
    glimpse = O.st_read(c["img"].double().repeat(c["T"], 1, 1), where, (c["h"], c["w"]))
    gw, = torch.autograd.grad((glimpse * c["dglimpse"].double()).sum(), [where])
    torch.testing.assert_close(c["dwhere_r64"], gw, rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("i", [0, 4])
def test_backward_reference_of_dpre_equals_central_differences(i):
    """rows are independent, so every row is differenced at once: column j of all rows moves by +-h and each row's own share of the
    objective is differenced (differencing the sum over rows would lose seven digits of every row to the others)"""
    c = AC.bwd_case(i)
    ds = c["dwhere_w"].double().sum(0) + c["dwhere_r64"]
    dk = c["dkl_row"].double() if c["dkl_row"] is not None else torch.zeros(ds.shape[0], dtype=torch.float64)

    def rows(pre):
        head = AC.where_head64(pre, c["eps"].double())
        return (head["where"] * ds).sum(1) + AC.DKL_SCALE * dk * head["kl_row"]

    pre, h = c["pre"].double(), 1e-5
    fd = torch.empty_like(c["dpre64"])
    for j in range(8):
        e = torch.zeros(8, dtype=torch.float64); e[j] = h
        # Richardson step on the central difference: the h^2 term cancels, leaving h^4 f^(5) / 30
        d1 = (rows(pre + e) - rows(pre - e)) / (2 * h)
        d2 = (rows(pre + 2 * e) - rows(pre - 2 * e)) / (4 * h)
        fd[:, j] = (4 * d1 - d2) / 3
    torch.testing.assert_close(fd, c["dpre64"], rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("i", range(len(AC.WHAT_CASES)))
def test_what_case_builds_with_its_conditions(i):
    c = AC.what_case(i)
    M, A = c["T"] * c["B"], c["A"]
    assert c["q64"].shape == (M, 2 * A) and c["kl_row64"].shape == (M,)
    pack = AC.pack_ref(c["sample64"], c["where"].double(), c["presence"].double(), [s.double() for s in c["states"]], c["T"], c["B"])
    assert pack.shape == (c["B"], c["T"] * A + 5 * c["T"] + c["S0"] + c["S1"])
    # column t * A + a of row b is sample[t * B + b, a]
    assert float(pack[c["B"] - 1, (c["T"] - 1) * A + A - 1]) == float(c["sample64"][M - 1, A - 1])
    assert float(pack[0, c["T"] * A + 4 * c["T"]]) == float(c["presence"][0, 0])


def test_what_cases_reach_the_ragged_edges():
    cases = AC.WHAT_CASES
    assert any(c[4] % 8 for c in cases) and any(c[4] % 8 == 0 for c in cases) and any((c[0] * c[1]) % 16 for c in cases)
    assert any(c[3] > c[2] for c in cases) and any(c[8] for c in cases) and any(c[5] == 0 and c[6] == 0 for c in cases)
    assert any(c[1] * (5 * c[0] + c[5] + c[6]) > 65536 for c in cases) and any(c[7] == AC.BF16 for c in cases)
