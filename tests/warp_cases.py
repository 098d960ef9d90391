"""Case table, builders, float64 references, bounds, the float32 restatement and planted defects for the kernel-level tests of the
spatial transformer (tests/test_warp_kernels.py): the glimpse read (csrc/st_kernels.hip: st_read_fwd_kernel, st_read_fwd_lean_kernel
<NT, VEC>, st_read_bwd_kernel) and the canvas launches (csrc/canvas_kernels.hip: st_write_fwd_kernel, st_write_bwd_gs_kernel<RC, IM>,
canvas_fused_gs_kernel<SPLIT>).  Importable without a GPU; tests/test_warp_cases_host.py holds every row against the library's
host-only form queries (air_st_read_form, air_st_read_bwd_form, air_canvas_fwd_form, air_canvas_bwd_form, air_canvas_fwd_bwd_form),
checks the inputs' promises, the restatement's share of every bound, the defects' margins and that every reachable form has a row.
No test lives here.

Groups.  V air_st_read_fwd (bits against oracle/st_loops.c in float32); W air_st_read_bwd (dwhere, dimg against the same loops in
float64); X air_st_write_fwd / air_canvas_unroll_fwd / _banded (bits against the oracle's sequential accumulation; the reconstruction
shares, added in band order, against float64); Y air_st_write_bwd / air_canvas_unroll_bwd / _dpresence (dglimpse, dwhere, dpresence
against float64 autograd through oracle.air_oracle.st_write); Z air_canvas_unroll_fwd_bwd (forward bits as X, dglimpse bits as the
recompute form of Y, the sum of the dwhere slabs at Y's bound).

Transforms.  `where` rows are drawn on the CPU by rejection: a row is kept only if no sampling coordinate inside [-2, extent + 1], on
either axis (for the canvas: all W + H of them), lies closer to an integer than max(DELTA, 16 * 2^-24 * M), M = the sum of the
magnitudes of the coordinate's own summands -- d/dwhere jumps at a cell boundary, and a float32 coordinate on the other side of one
than its float64 value differentiates another cell.  (The second term only matters at extreme scales: at 1e-3 a coordinate is the
difference of two numbers near a thousand and float32 moves it by more than DELTA.)  Planted rows carry a small fixed translation
jitter, the first of JITTER that passes the same filter.  At most REDRAW_CAP of the draws of a shape may have to be redrawn.
The identity rows ([1, 0, 1, 0] with W == w: every coordinate an integer) are exempt: their cases are held bit for bit between forms
and against the FLOAT32 scalar oracle only (`identity` in the table).

Operands and outputs.  Every operand is a window of a NaN-filled parent, every output a NaN-primed window of a SENTINEL-filled parent;
`off` names the operands whose window starts 4 bytes past a 16-byte boundary.

Bounds.  Elementwise, from float64 quantities only: |out - out64| <= CONST[group] * 2^-24 * S, where S is the sum of the absolute
values of the summands of that element's analytic expression, plus the term through which a coordinate rounding of 2^-24 * M moves
the bilinear weights (every gradient here is a sum over weights formed from rounded coordinates, dglimpse included).  With
dcanvas formed from (final canvas, obs) it is the float64 expression of the float32 final canvas the launch is given -- the backward
is a function of that operand; the recompute forms re-create it bit for bit -- and the magnitudes of its own summands,
coef * (mult |final| + |obs|), stand in for |dcanvas|.  obs carries random signs like every other operand (a non-negative image makes
dcanvas nearly constant, and a constant telescopes out of d/dwhere: the values would be remnants of their summands).
An element with S == 0 (a glimpse off the canvas) must be exactly zero.  The constants come from the oracle evaluated in float32
on the same inputs (restatement), which must stay within RESTATEMENT_SHARE of every bound -- never from a GPU result."""
import functools

import numpy as np
import torch

from attend_cases import SENTINEL
from oracle import air_oracle as O
from oracle import st_loops as C

NAN = float("nan")
U32 = 2.0 ** -24
DELTA = 1e-3
REDRAW_CAP = 0.25
RESTATEMENT_SHARE = 0.25            # the project's figure (tests/gemm_cases.py)
DEFECT_MARGIN = 4.0
N_REF = 48                          # images per case that get a CPU reference; the others repeat them (b % N_REF) and are compared on the device
JITTER = (0.013, 0.017, 0.021, 0.009, 0.027, 0.031, 0.007, 0.037, 0.041, 0.023)
MULT, STD = 0.5, 0.3
# one constant per group: four times the worst ratio |oracle32 - oracle64| / (2^-24 S) of the group's comparisons, rounded up.  The
# worst ratios are 1.27 (W: dwhere of W_per_image), 0.59 (X: the reconstruction term of X_write_512's canvases), 0.83 (Y: Y_img_default)
# and 0.75 (Z: Z_516_items); tests/test_warp_cases_host.py prints them and asserts the share they leave.
CONST = {"W": 6.0, "X": 3.0, "Y": 4.0, "Z": 3.0}
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -5         # AIR_E_* of include/air_hip.h


# ---------------------------------------------------------------------------------------------------------------
# coordinates, the off-boundary filter, transforms
# ---------------------------------------------------------------------------------------------------------------
def lin64(n):
    return np.linspace(-1.0, 1.0, n) if n > 1 else np.array([-1.0])


def axis_ab(where, kind, axis):
    """the affine map of one axis, coord = cs * ((a * X + b) + 1): read a = s, b = t; write (the inverse warp) a = 1/s, b = -t/s"""
    s = np.asarray(where, np.float64)[:, 0 + 2 * axis]
    t = np.asarray(where, np.float64)[:, 1 + 2 * axis]
    return (s, t) if kind == "read" else (1.0 / s, -t / s)


def coords64(where, kind, axis, n_pts, n_src):
    """-> coordinates [n, n_pts] in source cells and M [n, n_pts], the sum of the magnitudes of their summands"""
    a, b = axis_ab(where, kind, axis)
    X, cs = lin64(n_pts), (n_src - 1) / 2.0
    c = cs * ((a[:, None] * X[None] + b[:, None]) + 1.0)
    return c, cs * (np.abs(a[:, None] * X[None]) + np.abs(b[:, None]) + 1.0)


def _dims(kind, H, W, h, w):
    """(n_pts, n_src) of the x and the y axis: the read samples the image at glimpse points, the write the glimpse at canvas points"""
    return ((w, W), (h, H)) if kind == "read" else ((W, w), (H, h))


def boundary_distance(where, kind, H, W, h, w):
    """per row: the smallest of dist(coordinate, nearest integer) - max(DELTA, 16 * 2^-24 * M) over the coordinates inside
    [-2, extent + 1] of both axes (+inf when there is none), and the same with DELTA alone"""
    worst = np.full(len(where), np.inf)
    plain = np.full(len(where), np.inf)
    for axis, (n_pts, n_src) in enumerate(_dims(kind, H, W, h, w)):
        c, M = coords64(where, kind, axis, n_pts, n_src)
        near = (c >= -2.0) & (c <= n_src + 1.0)
        dist = np.abs(c - np.round(c))
        worst = np.minimum(worst, np.where(near, dist - np.maximum(DELTA, 16 * U32 * M), np.inf).min(1))
        plain = np.minimum(plain, np.where(near, dist - DELTA, np.inf).min(1))
    return worst, plain


def off_boundary(where, kind, H, W, h, w):
    return boundary_distance(where, kind, H, W, h, w)[0] > 0


DRAWS = {}                          # (kind, H, W, h, w) -> [draws, redraws], filled by draw_where


def draw_where(n, kind, H, W, h, w, rng):
    """n rows [sx, tx, sy, ty] (float32 values), sx of either sign, kept by the off-boundary filter"""
    out = np.empty((n, 4), np.float32)
    cnt = DRAWS.setdefault((kind, H, W, h, w), [0, 0])
    todo = np.arange(n)
    while len(todo):
        m = len(todo)
        rows = np.stack([rng.uniform(0.2, 1.4, m) * rng.choice([-1.0, 1.0], m), rng.uniform(-0.8, 0.8, m),
                         rng.uniform(0.2, 1.4, m), rng.uniform(-0.8, 0.8, m)], 1).astype(np.float32)
        ok = off_boundary(rows, kind, H, W, h, w)
        out[todo[ok]] = rows[ok]
        cnt[0] += m
        cnt[1] += int((~ok).sum())
        todo = todo[~ok]
    return out


def jittered(row, kind, H, W, h, w, jscale=1.0):
    """a planted row with the first translation jitter of JITTER (x) / its successor (y) that passes the filter (jscale: the jitter in
    units of the row's own extent where that is tiny)"""
    for i in range(len(JITTER) ** 2):
        jx, jy = jscale * JITTER[i % len(JITTER)], jscale * JITTER[(i // len(JITTER) + i + 1) % len(JITTER)]
        r = np.array([[row[0], row[1] + jx, row[2], row[3] + jy]], np.float32)
        if off_boundary(r, kind, H, W, h, w)[0]:
            return r[0]
    raise AssertionError(("no jitter passes the filter", row, kind, H, W, h, w))


def touched_counts(where_row, W, w):
    """float64 restatement of the canvas kernels' column ranges for one row -> (touched[w], candidates[w]): the canvas columns whose
    taps touch glimpse column j (floor in {j - 1, j}), and the size of src_range's candidate interval for it (st_device.h)"""
    c, _ = coords64(where_row[None], "write", 0, W, w)
    c = c[0]
    valid = (c > -1) & (c < w)
    f = np.floor(c)
    s, t = float(where_row[0]), float(where_row[1])
    b, cs, half = -t / s, (w - 1) / 2.0, 0.5 * (W - 1)
    touched, cand = [], []
    for j in range(w):
        touched.append(int((valid & ((f == j) | (f + 1 == j))).sum()))
        J0 = (((j - 1) / cs - 1.0) - b) * s + 1.0
        J1 = (((j + 1) / cs - 1.0) - b) * s + 1.0
        lo, hi = min(J0, J1) * half, max(J0, J1) * half
        a0, a1 = int(np.floor(lo)) - 1, int(np.ceil(hi)) + 1
        a0 = min(max(a0, 0), W - 1)
        a1 = max(min(a1, W - 1), 0)
        cand.append(a1 - a0 + 1)
    return np.array(touched), np.array(cand)


# spans of a glimpse cell in canvas columns, 2 r = 2 s (W - 1) / (w - 1): 4.0 -> four touched columns and eight candidates, 5.0 -> five
# and nine; 3.6 -> at most eight candidates; 4.4 -> nine in some columns (the general loop) while others keep eight
COUNT_ROWS = {"touch4": 4.0, "touch5": 5.0, "cand8": 3.6, "cand9": 4.4}


def planted_rows(kind, H, W, h, w, counts=False):
    """name -> row.  Read and write: mirrored on one / both axes, scale 1e-3 (write: the whole glimpse inside one canvas pixel whose
    centre it covers; read: every sample inside one image cell), scales 25 and 40, far off (exactly zero), the glimpse smaller than two
    canvas pixels; counts (write, shapes that admit them): the four rows of COUNT_ROWS"""
    X, Y = lin64(W), lin64(H)
    rows = {
        "mirror_x": [-0.7, 0.2, 0.9, -0.13], "mirror_xy": [-0.8, -0.1, -0.6, 0.15],
        "tiny": [1e-3, X[W // 2] + 3e-4, 1e-3, Y[H // 3] - 4e-4] if kind == "write" else [1e-3, 0.1, 1e-3, -0.2],
        "scale25": [25.0, 0.1, 25.0, -0.2], "scale40": [40.0, -0.3, 40.0, 0.2],
        "far": [0.3, 5.0, 0.3, 0.0], "small": [0.04, 0.1, 0.05, -0.3],
    }
    if counts:
        for name, r2 in COUNT_ROWS.items():
            rows[name] = [0.5 * r2 * (w - 1) / (W - 1), 0.0, 0.5 * r2 * (h - 1) / (H - 1), 0.0]
    return {k: jittered(v, kind, H, W, h, w, 1e-2 if (k, kind) == ("tiny", "write") else 1.0) for k, v in rows.items()}


# ---------------------------------------------------------------------------------------------------------------
# windows into NaN / sentinel parents
# ---------------------------------------------------------------------------------------------------------------
class Win:
    """a contiguous window of a flat parent: 8 (+1 when `off`) floats in front, 8 behind.  The parent's base is aligned far beyond 16
    bytes (host: the fake address BASE; device: the allocator's), so `off` alone decides the window's 16-byte alignment."""
    BASE = 1 << 24

    def __init__(self, shape, off=False, fill=NAN, inner=None):
        self.shape, self.lead = tuple(shape), 8 + int(bool(off))
        self.n = int(np.prod(self.shape))
        self.parent = torch.full((self.lead + self.n + 8,), fill, dtype=torch.float32)
        self.v = self.parent[self.lead:self.lead + self.n].view(self.shape)
        if inner is not None:
            self.v.fill_(inner)

    def addr(self):
        return Win.BASE + 4 * self.lead

    def cuda(self):
        """-> (device parent, device window)"""
        p = self.parent.cuda()
        return p, p[self.lead:self.lead + self.n].view(self.shape)


def out_win(shape, off=False):
    """an output: NaN-primed window of a SENTINEL parent"""
    return Win(shape, off, SENTINEL, NAN)


def surroundings_intact(win, dev_parent):
    p = dev_parent.detach().cpu()
    edge = torch.cat([p[:win.lead], p[win.lead + win.n:]])
    return bool((edge.view(torch.int32) == torch.full_like(edge, SENTINEL).view(torch.int32)).all())


# ---------------------------------------------------------------------------------------------------------------
# the separable bilinear map in float64: out[k] = Wy[k] . src[k] . Wx[k]^T, its gradients and the S of each
# ---------------------------------------------------------------------------------------------------------------
def axis64(a, b, n_pts, n_src, drop=None, neighbour=False):
    """-> Wm [K, n_pts, n_src] weights, D [K, n_pts, n_src] their derivative along the coordinate, M [K, n_pts], X [n_pts], cs.
    Defects: drop = (k, q, j): point q of unit k is left out of source index j's range; neighbour: unit 0 takes each weight from the
    next point's entry"""
    X, cs = lin64(n_pts), (n_src - 1) / 2.0
    c = cs * ((a[:, None] * X[None] + b[:, None]) + 1.0)
    M = cs * (np.abs(a[:, None] * X[None]) + np.abs(b[:, None]) + 1.0)
    valid = (c > -1) & (c < n_src)
    f = np.floor(np.where(valid, c, 0.0))
    d = f + 1.0 - np.where(valid, c, 0.0)
    if neighbour:
        d = d.copy()
        d[0, :-1] = d[0, 1:]
    Wm = np.zeros(c.shape + (n_src,))
    D = np.zeros_like(Wm)
    idx = np.arange(n_src)
    for tap, wgt, dw in ((f, d, -1.0), (f + 1, 1.0 - d, 1.0)):
        ok = valid & (tap >= 0) & (tap <= n_src - 1)
        hit = ok[..., None] & (tap[..., None] == idx)
        Wm += np.where(hit, wgt[..., None], 0.0)
        D += np.where(hit, dw, 0.0)
    if drop is not None:
        Wm[drop] = 0.0
        D[drop] = 0.0
    return Wm, D, M, X, cs


def warp64(src, ax, bx, ay, by, nx, ny, gout, gabs=None, **defect):
    """src [K, sy, sx], gout [K, ny, nx] (gabs: the magnitude that stands in for |gout| in S) ->
    dict: out, dsrc, dab [K, 4] = d/d(ax, bx, ay, by), dscal [K] = sum gout0 * out (gout0 = gout), and S_dsrc, S_dab, S_scal"""
    K, sy, sx = src.shape
    Wx, Dx, Mx, X, csx = axis64(ax, bx, nx, sx, drop=defect.get("drop_x"), neighbour=defect.get("neighbour", False))
    Wy, Dy, My, Y, csy = axis64(ay, by, ny, sy)
    gabs = np.abs(gout) if gabs is None else gabs
    A = np.abs(src)
    aDx, aDy = np.abs(Dx) * Mx[..., None], np.abs(Dy) * My[..., None]          # |dW| * coordinate rounding, in units of 2^-24
    e = lambda *ops: np.einsum(*ops, optimize=True)
    r = {"out": e("kIi,kij,kJj->kIJ", Wy, src, Wx)}
    r["dsrc"] = e("kIi,kIJ,kJj->kij", Wy, gout, Wx)
    r["P_dsrc"] = e("kIi,kIJ,kJj->kij", Wy, gabs, Wx)                         # (P_*: the summands alone, without the coordinate term)
    r["S_dsrc"] = (r["P_dsrc"] + e("kIi,kIJ,kJj->kij", aDy, gabs, Wx) + e("kIi,kIJ,kJj->kij", Wy, gabs, aDx))
    gx = e("kIi,kij,kJj->kIJ", Wy, src, Dx)                                    # d out / d x
    gy = e("kIi,kij,kJj->kIJ", Dy, src, Wx)
    Sgx = e("kIi,kij,kJj->kIJ", Wy + aDy, A, np.abs(Dx))
    Sgy = e("kIi,kij,kJj->kIJ", np.abs(Dy), A, Wx + aDx)
    r["dab"] = np.stack([csx * (gout * gx * X[None, None, :]).sum((1, 2)), csx * (gout * gx).sum((1, 2)),
                         csy * (gout * gy * Y[None, :, None]).sum((1, 2)), csy * (gout * gy).sum((1, 2))], 1)
    r["S_dab"] = np.stack([csx * (gabs * Sgx * np.abs(X)[None, None, :]).sum((1, 2)), csx * (gabs * Sgx).sum((1, 2)),
                           csy * (gabs * Sgy * np.abs(Y)[None, :, None]).sum((1, 2)), csy * (gabs * Sgy).sum((1, 2))], 1)
    Pgx, Pgy = e("kIi,kij,kJj->kIJ", Wy, A, np.abs(Dx)), e("kIi,kij,kJj->kIJ", np.abs(Dy), A, Wx)
    r["P_dab"] = np.stack([csx * (gabs * Pgx * np.abs(X)[None, None, :]).sum((1, 2)), csx * (gabs * Pgx).sum((1, 2)),
                           csy * (gabs * Pgy * np.abs(Y)[None, :, None]).sum((1, 2)), csy * (gabs * Pgy).sum((1, 2))], 1)
    r["S_out"] = e("kIi,kij,kJj->kIJ", Wy, A, Wx)
    r["S_out_coord"] = r["S_out"] + e("kIi,kij,kJj->kIJ", aDy, A, Wx) + e("kIi,kij,kJj->kIJ", Wy, A, aDx)
    return r


def chain_write(where, dab, S_dab, no_s2=False):
    """d/d(a, b) of the inverse warp (a = 1/s, b = -t/s) -> d/d(s, t) per axis, and its S.  Defect no_s2: the 1/s^2 factor left out"""
    wh = np.asarray(where, np.float64)
    dw, S = np.empty_like(dab), np.empty_like(dab)
    for ax in (0, 1):
        s, t = wh[:, 2 * ax], wh[:, 2 * ax + 1]
        s2 = np.ones_like(s) if no_s2 else s * s
        dw[:, 2 * ax] = (-dab[:, 2 * ax] + t * dab[:, 2 * ax + 1]) / s2
        dw[:, 2 * ax + 1] = -dab[:, 2 * ax + 1] / s
        S[:, 2 * ax] = (S_dab[:, 2 * ax] + np.abs(t) * S_dab[:, 2 * ax + 1]) / (s * s)
        S[:, 2 * ax + 1] = S_dab[:, 2 * ax + 1] / np.abs(s)
    return dw, S


def read_bwd64(img, where, dout, **defect):
    """img [K, H, W] (already gathered per glimpse), where [K, 4], dout [K, h, w] -> dwhere, dimg (per glimpse), S_dwhere, S_dimg"""
    ax, bx = axis_ab(where, "read", 0)
    ay, by = axis_ab(where, "read", 1)
    r = warp64(img.astype(np.float64), ax, bx, ay, by, dout.shape[2], dout.shape[1], dout.astype(np.float64), **defect)
    return r["dab"], r["dsrc"], r["S_dab"], r["S_dsrc"]


def write_bwd64(glm, where, pres, dc, dc_abs=None, H=None, W=None, **defect):
    """analytic float64 backward of canvas += p * inverse_warp(glimpse) for K units: glm [K, h, w], where [K, 4], pres [K], dc [K, H, W]
    (dc_abs: the magnitude of dc's own summands).  -> dict dglimpse, dwhere, dpresence and S_* of each.
    Defects: drop_x / neighbour (axis64), no_s2 (chain_write), border = v: the zero border of the glimpse holds v"""
    ax, bx = axis_ab(where, "write", 0)
    ay, by = axis_ab(where, "write", 1)
    p = pres.astype(np.float64)[:, None, None]
    dc = dc.astype(np.float64)
    dc_abs = np.abs(dc) if dc_abs is None else dc_abs
    src = glm.astype(np.float64)
    border = defect.pop("border", None)
    no_s2 = defect.pop("no_s2", False)
    if border is not None:                                  # a bordered copy, the coordinates shifted by one cell: same map, other source
        K, h, w = src.shape
        big = np.full((K, h + 2, w + 2), float(border))
        big[:, 1:-1, 1:-1] = src
        return _write_bwd_bordered(big, where, p, dc, H, W)
    r = warp64(src, ax, bx, ay, by, dc.shape[2], dc.shape[1], p * dc, np.abs(p) * dc_abs, **defect)
    dw, S_dw = chain_write(where, r["dab"], r["S_dab"], no_s2=no_s2)
    _, P_dw = chain_write(where, r["dab"], r["P_dab"])
    return dict(dglimpse=r["dsrc"], S_dglimpse=r["S_dsrc"], P_dglimpse=r["P_dsrc"], dwhere=dw, S_dwhere=S_dw, P_dwhere=P_dw,
                out=r["out"], S_out=r["S_out"], dpresence=(dc * r["out"]).sum((1, 2)),
                S_dpresence=(dc_abs * r["S_out_coord"]).sum((1, 2)), P_dpresence=(dc_abs * r["S_out"]).sum((1, 2)))


def _write_bwd_bordered(big, where, p, dc, H, W):
    """the defect `border`: dwhere and dpresence when the taps outside the glimpse read `border` instead of zero (dglimpse of the real
    elements is unchanged): the same separable map on the (h + 2) x (w + 2) source with coordinates one cell further, restricted to the
    points the true map accepts (-1 < coord < extent)"""
    K, h2, w2 = big.shape
    h, w = h2 - 2, w2 - 2
    outs = {}
    tabs = []
    for axis, (n_pts, n_src) in enumerate(((W, w), (H, h))):
        a, b = axis_ab(where, "write", axis)
        X, cs = lin64(n_pts), (n_src - 1) / 2.0
        c = cs * ((a[:, None] * X[None] + b[:, None]) + 1.0)
        valid = (c > -1) & (c < n_src)
        cc = np.where(valid, c, 0.0) + 1.0
        f = np.floor(cc)
        d = f + 1.0 - cc
        idx = np.arange(n_src + 2)
        Wm = np.where(valid[..., None] & (f[..., None] == idx), d[..., None], 0.0) + np.where(valid[..., None] & (f[..., None] + 1 == idx), 1.0 - d[..., None], 0.0)
        D = np.where(valid[..., None] & (f[..., None] == idx), -1.0, 0.0) + np.where(valid[..., None] & (f[..., None] + 1 == idx), 1.0, 0.0)
        tabs.append((Wm, D, X, cs))
    (Wx, Dx, X, csx), (Wy, Dy, Y, csy) = tabs
    e = lambda *ops: np.einsum(*ops, optimize=True)
    gout = p * dc
    gx, gy = e("kIi,kij,kJj->kIJ", Wy, big, Dx), e("kIi,kij,kJj->kIJ", Dy, big, Wx)
    dab = np.stack([csx * (gout * gx * X[None, None, :]).sum((1, 2)), csx * (gout * gx).sum((1, 2)),
                    csy * (gout * gy * Y[None, :, None]).sum((1, 2)), csy * (gout * gy).sum((1, 2))], 1)
    outs["dwhere"], _ = chain_write(where, dab, np.abs(dab))
    outs["dpresence"] = (dc * e("kIi,kij,kJj->kIJ", Wy, big, Wx)).sum((1, 2))
    return outs


# ---------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------
CASES = {}


def _case(name, group, entry, dims, form, **kw):
    """dims: V / W (n_img, R, H, W, h, w); X / Y / Z (T, B, H, W, h, w).  form: the fields of AirWarpForm the row expects (kernel by
    name), or the status the launch refuses with (`refused`: then no output may be written).  kw: see the builders"""
    assert name not in CASES, name
    assert group in "VWXYZ"
    CASES[name] = dict(name=name, group=group, entry=entry, dims=tuple(dims), form=form, off=kw.pop("off", ()), **kw)


def _lean(nt, vec, R, threads, **kw):
    return dict(kernel="read_fwd_lean", NT=nt, VEC=vec, R=R, threads=threads, vec4=1, **kw)


# ---- V. air_st_read_fwd -----------------------------------------------------------------------------------------------------------
_case("V_generic_narrow", "V", "read_fwd", (5, 2, 8, 3, 4, 4), dict(kernel="read_fwd", vec4=1, threads=256))            # W < 4
_case("V_generic_odd", "V", "read_fwd", (5, 1, 7, 5, 3, 3), dict(kernel="read_fwd", vec4=0))                            # H * W % 4 != 0
_case("V_generic_where_off", "V", "read_fwd", (4, 2, 8, 8, 4, 4), dict(kernel="read_fwd", vec4=1), off=("where",))
_case("V_generic_img_off", "V", "read_fwd", (4, 2, 8, 8, 4, 4), dict(kernel="read_fwd", vec4=0), off=("img",))
_case("V_lean_r1", "V", "read_fwd", (6, 1, 8, 8, 4, 4), _lean(0, 0, 1, 256))
_case("V_lean_w5", "V", "read_fwd", (6, 2, 8, 8, 4, 5), _lean(0, 0, 1, 256))
_case("V_lean_glimpse_off", "V", "read_fwd", (6, 2, 8, 8, 4, 4), _lean(0, 0, 1, 256), off=("glimpse",))
for _R in (2, 3, 4, 5):
    _case(f"V_lean_vec_r{_R}", "V", "read_fwd", (3, _R, 12, 10, 4, 8), _lean(0, 1, _R, 256))
_case("V_lean_nq768", "V", "read_fwd", (3, 2, 48, 64, 4, 4), _lean(0, 1, 2, 256))
_case("V_lean_nq770", "V", "read_fwd", (3, 2, 55, 56, 4, 4), _lean(0, 1, 2, 1024))
_case("V_lean_nq3072", "V", "read_fwd", (2, 2, 96, 128, 4, 4), _lean(0, 1, 2, 1024))
_case("V_generic_nq3073", "V", "read_fwd", (2, 2, 28, 439, 4, 4), dict(kernel="read_fwd", vec4=1))
_case("V_identity", "V", "read_fwd", (3, 1, 8, 8, 8, 8), _lean(0, 0, 1, 256), identity=True)
# streaming: 4 * (n_img * 96 * 128 + n * 16) bytes first exceed 64 MiB at 1364 images with one glimpse each, 1362 with two
_case("V_stream_r1", "V", "read_fwd", (1364, 1, 96, 128, 4, 4), _lean(1, 0, 1, 1024, resident_cap=0))
_case("V_stream_vec", "V", "read_fwd", (1362, 2, 96, 128, 4, 4), _lean(1, 1, 2, 1024))
_case("V_grid_stride", "V", "read_fwd", (2100, 2, 7, 8, 2, 4), _lean(0, 1, 2, 256, resident_cap=1))
_case("V_refuse_null", "V", "read_fwd", (2, 1, 8, 8, 4, 4), dict(refused=E_NULL), null=("where",))
_case("V_refuse_dims", "V", "read_fwd", (2, 1, 8, 8, 0, 4), dict(refused=E_SHAPE))
_case("V_refuse_share", "V", "read_fwd", (2, 1.5, 8, 8, 4, 4), dict(refused=E_SHAPE))                                   # n % n_img != 0
_case("V_refuse_lds", "V", "read_fwd", (1, 1, 210, 200, 2, 2), dict(refused=E_UNSUPPORTED))

# ---- W. air_st_read_bwd ------------------------------------------------------------------------------------------------------------
_rb = lambda pg, v4, **kw: dict(kernel="read_bwd", per_glimpse=pg, vec4=v4, threads=256, **kw)
_case("W_per_glimpse_odd", "W", "read_bwd", (4, 3, 13, 17, 5, 7), _rb(1, 0))
_case("W_per_glimpse_vec4", "W", "read_bwd", (4, 3, 12, 16, 5, 7), _rb(1, 1))
_case("W_per_image", "W", "read_bwd", (12, 1, 12, 16, 5, 7), _rb(0, 1))
_case("W_per_image_dimg", "W", "read_bwd", (12, 1, 12, 16, 5, 7), _rb(0, 1), dimg=True)
_case("W_dimg_img_off", "W", "read_bwd", (12, 1, 12, 16, 6, 4), _rb(0, 0), dimg=True, off=("img",))
_case("W_shared_2048", "W", "read_bwd", (1024, 2, 7, 5, 2, 3), _rb(1, 0, items=2048, resident_cap=0))
_case("W_shared_2049", "W", "read_bwd", (683, 3, 7, 5, 2, 3), _rb(0, 0, items=683))
_case("W_identity", "W", "read_bwd", (3, 1, 8, 8, 8, 8), _rb(0, 1), dimg=True, identity=True)
_case("W_refuse_dimg_shared", "W", "read_bwd", (4, 3, 12, 16, 5, 7), dict(refused=E_UNSUPPORTED), dimg=True)
_case("W_refuse_null", "W", "read_bwd", (4, 1, 12, 16, 5, 7), dict(refused=E_NULL), null=("dglimpse",))
_case("W_refuse_dims", "W", "read_bwd", (4, 1, 12, -1, 5, 7), dict(refused=E_SHAPE))
_case("W_refuse_lds", "W", "read_bwd", (1, 1, 150, 140, 2, 2), dict(refused=E_UNSUPPORTED), dimg=True)

# ---- X. the canvas forward ------------------------------------------------------------------------------------------------------
# entry "write_fwd": air_st_write_fwd (T = 1); "unroll_fwd": air_canvas_unroll_fwd (its own band rule); "banded": _fwd_banded.
# pres: "binary" (cumulative), "cont" (0.2, 1), None (NULL: ones); outs: which of canvas_steps / final_canvas are asked for; rec: the
# reconstruction shares; canvas_in (write_fwd only)
_wf = lambda thr, NB, RB, v4g=1, **kw: dict(kernel="write_fwd", threads=thr, NB=NB, RB=RB, vec4_glimpse=v4g, **kw)
_case("X_write_px_small", "X", "write_fwd", (1, 5, 7, 5, 2, 2), _wf(64, 1, 7, 0), pres=None, canvas_in=False)           # px = 35 < 64
_case("X_write_canvas_in", "X", "write_fwd", (1, 5, 17, 13, 5, 7), _wf(256, 1, 17, 0), pres="cont", canvas_in=True)
_case("X_write_px_1024", "X", "write_fwd", (1, 3, 50, 50, 20, 20), _wf(1024, 1, 50), pres="binary", canvas_in=True)
_case("X_write_glimpse_off", "X", "write_fwd", (1, 3, 21, 19, 6, 8), _wf(448, 1, 21, 0), pres=None, canvas_in=False, off=("glimpse",))
_case("X_write_257", "X", "write_fwd", (1, 257, 7, 5, 3, 2), _wf(512, 1, 7, 0, items=257), pres="cont", canvas_in=False)
_case("X_write_512", "X", "write_fwd", (1, 512, 7, 5, 3, 2), _wf(512, 1, 7, 0), pres="cont", canvas_in=True)
_case("X_write_513", "X", "write_fwd", (1, 513, 7, 5, 3, 2), _wf(256, 1, 7, 0), pres=None, canvas_in=False)
_case("X_write_stride", "X", "write_fwd", (1, 2100, 7, 5, 2, 4), _wf(256, 1, 7, 1, resident_cap=1), pres="binary", canvas_in=False)
_case("X_write_identity", "X", "write_fwd", (1, 3, 8, 8, 8, 8), _wf(64, 1, 8), pres=None, canvas_in=False, identity=True)
_case("X_unroll_own_bands", "X", "unroll_fwd", (3, 6, 50, 50, 20, 20), _wf(128, 25, 2), pres="binary", outs="both", rec=False)   # 256 / 6 = 42 bands asked, 25 of two rows kept
_case("X_unroll_rec", "X", "unroll_fwd", (3, 6, 50, 50, 20, 20), _wf(1024, 1, 50), pres="binary", outs="both", rec=True)
_case("X_banded_2", "X", "banded", (3, 3, 50, 50, 20, 20), _wf(1024, 2, 25), pres="cont", outs="final", rec=True, n_bands=2)
_case("X_banded_8", "X", "banded", (2, 2, 50, 50, 20, 20), _wf(384, 8, 7), pres=None, outs="steps", rec=True, n_bands=8)
_case("X_banded_unkept", "X", "banded", (2, 3, 7, 5, 2, 2), _wf(64, 4, 2, 0), pres="binary", outs="both", rec=False, n_bands=5)
_case("X_banded_unkept_rec", "X", "banded", (2, 3, 7, 5, 2, 2), dict(refused=E_SHAPE), pres="binary", outs="both", rec=True, n_bands=5)
_case("X_unroll_t9", "X", "unroll_fwd", (9, 4, 17, 13, 3, 5), _wf(256, 1, 17, 0), pres="binary", outs="both", rec=True)
_case("X_unroll_t32", "X", "unroll_fwd", (32, 3, 12, 10, 2, 4), _wf(128, 1, 12, 1), pres="cont", outs="final", rec=True)
_case("X_unroll_t32_off", "X", "unroll_fwd", (32, 3, 12, 10, 2, 4), _wf(128, 1, 12, 0), pres="binary", outs="steps", rec=True, off=("glimpse",))
_case("X_refuse_null", "X", "unroll_fwd", (2, 3, 7, 5, 2, 2), dict(refused=E_NULL), pres="binary", outs="none", rec=False)
_case("X_refuse_rec_no_obs", "X", "unroll_fwd", (2, 3, 7, 5, 2, 2), dict(refused=E_NULL), pres="binary", outs="both", rec=True, null=("obs",))
_case("X_refuse_t0", "X", "unroll_fwd", (0, 3, 7, 5, 2, 2), dict(refused=E_SHAPE), pres="binary", outs="both", rec=False)
_case("X_refuse_dims", "X", "write_fwd", (1, 3, 7, 0, 2, 2), dict(refused=E_SHAPE), pres=None, canvas_in=False)
_case("X_refuse_lds", "X", "unroll_fwd", (32, 1, 12, 10, 40, 40), dict(refused=E_UNSUPPORTED), pres="binary", outs="both", rec=False)

# ---- Y. the canvas backward ------------------------------------------------------------------------------------------------------
# entry "write_bwd": air_st_write_bwd (dcanvas given, T = 1); "unroll_bwd" / "unroll_bwd_dp": air_canvas_unroll_bwd / _dpresence with
# variant "stored" (final canvas read) or "recompute" (final_canvas = NULL).  env: the per-call switches the row runs under.
# Every stored row is also run as recompute and the two compared for bits; every image-major row also unit-major (AIR_CANVAS_BWD_IMG=0).
_wb = lambda rc, im, thr, v4g=1, v4c=1, **kw: dict(kernel="write_bwd", RC=rc, IM=im, threads=thr, vec4_glimpse=v4g, vec4_canvas=v4c, **kw)
IMG0 = {"AIR_CANVAS_IMG_MIN_UNITS": "0"}
_case("Y_dcanvas", "Y", "write_bwd", (1, 20, 50, 50, 20, 20), _wb(0, 0, 512), pres="cont", dp=True, counts=True)
_case("Y_dcanvas_odd", "Y", "write_bwd", (1, 12, 17, 13, 5, 7), _wb(0, 0, 512, 0, 0), pres=None, dp=False)
_case("Y_dcanvas_off", "Y", "write_bwd", (1, 12, 12, 10, 4, 4), _wb(0, 0, 512, 1, 0), pres="binary", dp=True, off=("dcanvas",))
_case("Y_dcanvas_identity", "Y", "write_bwd", (1, 3, 8, 8, 8, 8), _wb(0, 0, 512), pres=None, dp=False, identity=True)
# the identity through the unrolled entry: image-major, then (by the test) unit-major on purpose and the recompute form, bit for bit
_case("Y_unroll_identity", "Y", "unroll_bwd_dp", (2, 3, 8, 8, 8, 8), _wb(0, 1, 256), pres="cont", variant="stored", env=IMG0, identity=True)
_case("Y_stored", "Y", "unroll_bwd", (3, 8, 50, 50, 20, 20), _wb(0, 0, 512), pres="binary", variant="stored", counts=True)
_case("Y_stored_dp", "Y", "unroll_bwd_dp", (3, 8, 21, 19, 6, 10), _wb(0, 0, 512, 0, 0), pres="cont", variant="stored")
_case("Y_recompute", "Y", "unroll_bwd", (3, 8, 50, 50, 20, 20), _wb(1, 0, 512), pres="binary", variant="recompute", counts=True)
_case("Y_stored_obs_off", "Y", "unroll_bwd", (2, 9, 12, 10, 4, 4), _wb(0, 0, 512, 1, 0), pres="cont", variant="stored", off=("obs",))
_case("Y_stored_final_off", "Y", "unroll_bwd", (2, 9, 12, 10, 4, 4), _wb(0, 0, 512, 1, 0), pres="cont", variant="stored", off=("final",))
_case("Y_recompute_glimpse_off", "Y", "unroll_bwd", (2, 9, 12, 10, 4, 4), _wb(1, 0, 512, 0, 1), pres="binary", variant="recompute", off=("glimpse",))
for _thr in (128, 256, 512, 1024):
    _e = {"AIR_CANVAS_GS_THREADS": str(_thr)}
    _case(f"Y_unit_thr{_thr}", "Y", "unroll_bwd", (2, 6, 21, 19, 6, 10), _wb(0, 0, min(_thr, 512), 0, 0), pres="cont", variant="stored", env=_e)
    _case(f"Y_recompute_thr{_thr}", "Y", "unroll_bwd", (2, 6, 21, 19, 6, 10), _wb(1, 0, min(_thr, 512), 0, 0), pres="cont", variant="recompute", env=_e)
    _case(f"Y_img_thr{_thr}", "Y", "unroll_bwd", (2, 6, 21, 19, 6, 10), _wb(0, 1, _thr, 0, 0), pres="cont", variant="stored", env=dict(_e, **IMG0))
_case("Y_img_256", "Y", "unroll_bwd", (3, 6, 50, 50, 20, 20), _wb(0, 1, 256), pres="binary", variant="stored", env=IMG0, counts=True)
_case("Y_img_512", "Y", "unroll_bwd_dp", (5, 5, 50, 50, 20, 20), _wb(0, 1, 512), pres="cont", variant="stored", env=IMG0)
_case("Y_img_1024", "Y", "unroll_bwd", (8, 3, 56, 50, 20, 20), _wb(0, 1, 1024), pres="binary", variant="stored", env=IMG0)
# the image-major carve of 100 x 100 / 28 x 28 at T = 8 exceeds CV_MAX_LDS (the one shape beyond 50 x 50: no smaller one does): the
# query reports the unit-major form it falls back to, and the result equals that form launched on purpose (AIR_CANVAS_BWD_IMG=0), bit for bit
_case("Y_img_carve_falls_back", "Y", "unroll_bwd", (8, 2, 100, 100, 28, 28), _wb(0, 0, 512), pres="binary", variant="stored", env=IMG0)
_case("Y_img_t8", "Y", "unroll_bwd", (8, 3, 12, 10, 4, 4), _wb(0, 1, 256), pres="binary", variant="stored", env=IMG0)
_case("Y_img_t9_unit", "Y", "unroll_bwd", (9, 3, 12, 10, 4, 4), _wb(0, 0, 512), pres="binary", variant="stored", env=IMG0)
_case("Y_t32_unit", "Y", "unroll_bwd", (32, 3, 12, 10, 2, 4), _wb(0, 0, 512), pres="cont", variant="stored")
_case("Y_t32_recompute", "Y", "unroll_bwd", (32, 3, 12, 10, 2, 4), _wb(1, 0, 512), pres="cont", variant="recompute")
_case("Y_img_default", "Y", "unroll_bwd", (3, 700, 7, 5, 2, 4), _wb(0, 1, 256, 1, 0, items=700), pres="binary", variant="stored")
_case("Y_t9_stride", "Y", "unroll_bwd", (9, 230, 7, 5, 2, 4), _wb(0, 0, 256, 1, 0, resident_cap=1), pres="binary", variant="stored")
_case("Y_recompute_513", "Y", "unroll_bwd", (1, 513, 7, 5, 2, 4), _wb(1, 0, 256, 1, 0), pres="binary", variant="recompute")
_case("Y_refuse_null", "Y", "unroll_bwd", (2, 3, 7, 5, 2, 2), dict(refused=E_NULL), pres="binary", variant="stored", null=("dwhere",))
_case("Y_refuse_no_dp", "Y", "unroll_bwd_dp", (2, 3, 7, 5, 2, 2), dict(refused=E_NULL), pres="binary", variant="stored", null=("dpresence",))
_case("Y_refuse_t0", "Y", "unroll_bwd", (0, 3, 7, 5, 2, 2), dict(refused=E_SHAPE), pres="binary", variant="stored")
_case("Y_refuse_dims", "Y", "write_bwd", (1, 0, 7, 5, 2, 2), dict(refused=E_SHAPE), pres=None, dp=False)
_case("Y_refuse_lds", "Y", "unroll_bwd", (2, 1, 210, 200, 2, 2), dict(refused=E_UNSUPPORTED), pres="binary", variant="stored")

# ---- Z. air_canvas_unroll_fwd_bwd ------------------------------------------------------------------------------------------------
_fz = lambda split, ns, thr, NB, RB, v4g=1, v4c=1, **kw: dict(kernel="fused", RC=1, SPLIT=split, n_split=ns, threads=thr, NB=NB, RB=RB,
                                                              vec4_glimpse=v4g, vec4_canvas=v4c, **kw)
for _ns in (1, 2, 3, 4):
    _case(f"Z_split{_ns}", "Z", "fused", (3, 6, 50, 50, 20, 20), _fz(int(_ns > 1), _ns, 512, 4, 13), pres="binary", n_bands=4, n_split=_ns,
          counts=(_ns in (1, 4)))
_case("Z_identity", "Z", "fused", (2, 3, 8, 8, 8, 8), _fz(1, 2, 512, 2, 4), pres="cont", n_bands=2, n_split=2, identity=True)
_case("Z_identity_split1", "Z", "fused", (2, 3, 8, 8, 8, 8), _fz(0, 1, 512, 1, 8), pres="binary", n_bands=1, n_split=1, identity=True)
_case("Z_h2_split4", "Z", "fused", (2, 5, 17, 13, 2, 7), _fz(1, 4, 512, 2, 9, 0, 0), pres="cont", n_bands=2, n_split=4)
_case("Z_h3_split4", "Z", "fused", (2, 5, 12, 10, 3, 4), _fz(1, 4, 512, 1, 12), pres="binary", n_bands=1, n_split=4, off=())
_case("Z_512_items", "Z", "fused", (2, 128, 7, 5, 2, 4), _fz(1, 2, 512, 1, 7, 1, 0, items=128 + 512), pres="binary", n_bands=1, n_split=2)
_case("Z_516_items", "Z", "fused", (2, 129, 7, 5, 2, 4), _fz(1, 2, 256, 1, 7, 1, 0), pres="binary", n_bands=1, n_split=2)
_case("Z_limit_4096", "Z", "fused", (2, 1024, 7, 5, 2, 4), _fz(1, 2, 256, 4, 2, 1, 0, n_fwd=4096, items=8192), pres="binary", n_bands=4, n_split=2)
_case("Z_beyond_units", "Z", "fused", (2, 1025, 7, 5, 2, 4), dict(refused=E_UNSUPPORTED), pres="binary", n_bands=1, n_split=2)
_case("Z_beyond_bands", "Z", "fused", (1, 1025, 7, 5, 2, 4), dict(refused=E_UNSUPPORTED), pres="binary", n_bands=4, n_split=1)
_case("Z_obs_off", "Z", "fused", (2, 5, 12, 10, 4, 4), _fz(0, 1, 512, 2, 6, 1, 0), pres="cont", n_bands=2, n_split=1, off=("obs",))
_case("Z_glimpse_off", "Z", "fused", (2, 5, 12, 10, 4, 4), _fz(1, 3, 512, 2, 6, 0, 1), pres="cont", n_bands=2, n_split=3, off=("glimpse",))
_case("Z_refuse_null", "Z", "fused", (2, 3, 7, 5, 2, 2), dict(refused=E_NULL), pres="binary", n_bands=1, n_split=1, null=("rec_parts",))
_case("Z_refuse_split", "Z", "fused", (2, 3, 7, 5, 2, 2), dict(refused=E_SHAPE), pres="binary", n_bands=1, n_split=5)
_case("Z_refuse_bands", "Z", "fused", (2, 3, 7, 5, 2, 2), dict(refused=E_SHAPE), pres="binary", n_bands=5, n_split=1)
_case("Z_refuse_t0", "Z", "fused", (0, 3, 7, 5, 2, 2), dict(refused=E_SHAPE), pres="binary", n_bands=1, n_split=1)
_case("Z_refuse_lds", "Z", "fused", (32, 1, 12, 10, 40, 40), dict(refused=E_UNSUPPORTED), pres="binary", n_bands=1, n_split=1)

# NULL for each required pointer of each entry (the rows above hold one each already): status AIR_E_NULL, nothing written
for _grp, _entry, _shape, _kw, _ptrs in (
        ("V", "read_fwd", (2, 1, 8, 8, 4, 4), {}, ("img", "glimpse")),
        ("W", "read_bwd", (4, 1, 12, 16, 5, 7), {}, ("img", "where", "dwhere")),
        ("X", "write_fwd", (1, 3, 7, 5, 2, 2), dict(pres=None, canvas_in=False), ("glimpse", "where", "final")),
        ("X", "banded", (2, 3, 7, 5, 2, 2), dict(pres="binary", outs="both", rec=True, n_bands=1), ("glimpse", "where")),
        ("Y", "write_bwd", (1, 3, 7, 5, 2, 2), dict(pres=None, dp=False), ("glimpse", "where", "dcanvas", "dglimpse", "dwhere")),
        ("Y", "unroll_bwd", (2, 3, 7, 5, 2, 2), dict(pres="binary", variant="stored"), ("glimpse", "where", "obs", "dglimpse")),
        ("Z", "fused", (2, 3, 7, 5, 2, 2), dict(pres="binary", n_bands=1, n_split=1), ("glimpse", "where", "obs", "dglimpse", "dwhere"))):
    for _ptr in _ptrs:
        _case(f"{_grp}_null_{_entry}_{_ptr}", _grp, _entry, _shape, dict(refused=E_NULL), null=(_ptr,), **_kw)

# what the launch rules can reach: every kernel instantiation (1 + 4 + 1 + 1 + 3 + 2), every value of the staging flags, every
# workgroup size of every rule.  tests/test_warp_cases_host.py fails when a member is named by no row's expected form.
REACHABLE = (
    [("read_fwd",)] + [("read_fwd_lean", nt, vec) for nt in (0, 1) for vec in (0, 1)] + [("read_bwd",), ("write_fwd",)]
    + [("write_bwd", 0, 0), ("write_bwd", 1, 0), ("write_bwd", 0, 1), ("fused", 0), ("fused", 1)]
    + [("read_fwd", "vec4", v) for v in (0, 1)] + [("read_bwd", "vec4", v) for v in (0, 1)] + [("read_bwd", "per_glimpse", v) for v in (0, 1)]
    + [(k, f, v) for k in ("write_fwd", "write_bwd", "fused") for f in ("vec4_glimpse",) for v in (0, 1)]
    + [(k, "vec4_canvas", v) for k in ("write_bwd", "fused") for v in (0, 1)]
    + [("read_fwd_lean", "threads", t) for t in (256, 1024)]
    + [("write_fwd", "threads", t) for t in (64, 256, 512, 1024)]                      # the pixel rule's ends, 512 and 256 beyond it
    + [("write_bwd", "unit_threads", t) for t in (128, 256, 512)] + [("write_bwd", "recompute_threads", t) for t in (128, 256, 512)]
    + [("write_bwd", "image_threads", t) for t in (128, 256, 512, 1024)]
    + [("fused", "threads", t) for t in (256, 512)] + [("fused", "n_split", n) for n in (1, 2, 3, 4)]
)


def form_members(form):
    """the members of REACHABLE a form (dict over AirWarpForm's fields, kernel by name) names"""
    k = form["kernel"]
    out = set()
    if k == "read_fwd":
        out |= {(k,), (k, "vec4", form["vec4"])}
    elif k == "read_fwd_lean":
        out |= {(k, form["NT"], form["VEC"]), (k, "threads", form["threads"])}
    elif k == "read_bwd":
        out |= {(k,), (k, "vec4", form["vec4"]), (k, "per_glimpse", form["per_glimpse"])}
    elif k == "write_fwd":
        out |= {(k,), (k, "vec4_glimpse", form["vec4_glimpse"]), (k, "threads", form["threads"])}
    elif k == "write_bwd":
        rule = "recompute_threads" if form["RC"] else ("image_threads" if form["IM"] else "unit_threads")
        out |= {(k, form["RC"], form["IM"]), (k, "vec4_glimpse", form["vec4_glimpse"]), (k, "vec4_canvas", form["vec4_canvas"]),
                (k, rule, form["threads"])}
    elif k == "fused":
        out |= {(k, form["SPLIT"]), (k, "vec4_glimpse", form["vec4_glimpse"]), (k, "vec4_canvas", form["vec4_canvas"]),
                (k, "threads", form["threads"]), (k, "n_split", form["n_split"])}
    return out


# ---------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------
def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def _signed(rng, *shape):
    """magnitudes in [0.5, 1.5], random signs: no term can hide"""
    return (rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _presence(kind, T, B, rng):
    if kind is None:
        return None
    if kind == "cont":
        return rng.uniform(0.2, 1.0, (T, B)).astype(np.float32)
    p = np.cumprod(rng.integers(0, 2, (T, B)), 0).astype(np.float32)
    p[:, ::3] = 1.0                                         # every third image keeps all its steps
    if T > 1:
        p[-1, 1::3] = 0.0                                   # ... and the next one drops at least its last
    return p


def _periodic(a, n, axis):
    """a defined on N_REF members along `axis` -> n members, member i = a[i % N_REF]"""
    idx = np.arange(n) % min(n, N_REF)
    return np.ascontiguousarray(np.take(a, idx, axis))


def _where_write(case, T, B, H, W, h, w, rng):
    nb = min(B, N_REF)
    if case.get("identity"):
        return np.tile(np.array([1, 0, 1, 0], np.float32), (T, B, 1)), {}
    wh = draw_where(T * nb, "write", H, W, h, w, rng).reshape(T, nb, 4)
    planted = planted_rows("write", H, W, h, w, counts=case.get("counts", False))
    at = {}
    for i, (name, row) in enumerate(planted.items()):
        t, b = i % T, (i // T) % nb
        if (t, b) in at.values():
            continue
        wh[t, b] = row
        at[name] = (t, b)
    return _periodic(wh, B, 1), at


@functools.lru_cache(maxsize=None)
def data(name):
    """the case's operands (Win), references and S, on at most N_REF images (the others repeat them)"""
    case = CASES[name]
    rng = np.random.default_rng(_seed(name))
    off = set(case["off"])
    d = dict(case=case)
    if case["group"] in "VW":
        n_img, R, H, W, h, w = case["dims"]
        n = int(round(n_img * R))
        d.update(n=n, n_img=n_img)
        if "refused" in case["form"]:
            return d
        nb = min(n_img, N_REF)
        img = _signed(rng, nb, H, W)
        Rn = n // n_img
        if case.get("identity"):
            wh = np.tile(np.array([1, 0, 1, 0], np.float32), (Rn, nb, 1))
            at = {}
        else:
            wh = draw_where(Rn * nb, "read", H, W, h, w, rng).reshape(Rn, nb, 4)
            at = {}
            if case["group"] == "W":
                for i, (nm, row) in enumerate(planted_rows("read", H, W, h, w).items()):
                    r_, b_ = i % Rn, (i // Rn) % nb
                    if (r_, b_) not in at.values():
                        wh[r_, b_] = row
                        at[nm] = (r_, b_)
        d.update(img_ref=img, where_ref=wh, planted=at, nb=nb, R=Rn)
        d["img"] = Win((n_img, H, W), "img" in off)
        d["img"].v.copy_(torch.from_numpy(_periodic(img, n_img, 0)))
        d["where"] = Win((n, 4), "where" in off)
        d["where"].v.copy_(torch.from_numpy(_periodic(wh, n_img, 1).reshape(n, 4)))           # glimpse k = r * n_img + b reads image b
        gathered = np.broadcast_to(img[None], (Rn, nb, H, W)).reshape(Rn * nb, H, W)
        if case["group"] == "V":
            d["out32"] = C.st_read_fwd(np.ascontiguousarray(gathered), wh.reshape(-1, 4), (h, w)).reshape(Rn, nb, h, w)
        else:
            dout = _signed(rng, Rn, nb, h, w)
            d["dglimpse"] = Win((n, h, w), "dglimpse" in off)
            d["dglimpse"].v.copy_(torch.from_numpy(_periodic(dout, n_img, 1).reshape(n, h, w)))
            d.update(dout_ref=dout, gathered=gathered)
            f32 = C.st_read_bwd(np.ascontiguousarray(gathered), wh.reshape(-1, 4), dout.reshape(-1, h, w), want_dimg=True)
            d["dwhere32"], d["dimg32"] = f32[0].reshape(Rn, nb, 4), f32[1].reshape(Rn, nb, H, W)
            _, _, S_dw, S_di = read_bwd64(gathered, wh.reshape(-1, 4), dout.reshape(-1, h, w))
            d["S_dwhere"], d["S_dimg"] = S_dw.reshape(Rn, nb, 4), S_di.reshape(Rn, nb, H, W)
            if not case.get("identity"):
                f64 = C.st_read_bwd(np.ascontiguousarray(gathered.astype(np.float64)), wh.reshape(-1, 4).astype(np.float64),
                                    dout.reshape(-1, h, w).astype(np.float64), want_dimg=True)
                d["dwhere64"], d["dimg64"] = f64[0].reshape(Rn, nb, 4), f64[1].reshape(Rn, nb, H, W)
        return d
    # ---- canvas groups
    T, B, H, W, h, w = case["dims"]
    if "refused" in case["form"]:
        return d
    nb = min(B, N_REF)
    glm = _signed(rng, T, nb, h, w)
    wh, at = _where_write(case, T, B, H, W, h, w, rng)
    pres = _presence(case.get("pres"), T, nb, rng)
    if case.get("pres") == "binary":
        for t_, b_ in at.values():                          # a planted transform is a present step (cumulative: so are the steps before it)
            pres[:t_ + 1, b_] = 1.0
    obs = _signed(rng, nb, H, W)
    d.update(nb=nb, planted=at, glm_ref=glm, where_ref=wh[:, :nb], pres_ref=pres, obs_ref=obs)
    d["glimpse"] = Win((T, B, h, w), "glimpse" in off)
    d["glimpse"].v.copy_(torch.from_numpy(_periodic(glm, B, 1)))
    d["where"] = Win((T, B, 4), "where" in off)
    d["where"].v.copy_(torch.from_numpy(wh))
    if pres is not None:
        d["presence"] = Win((T, B))
        d["presence"].v.copy_(torch.from_numpy(_periodic(pres, B, 1)))
    d["obs"] = Win((B, H, W), "obs" in off)
    d["obs"].v.copy_(torch.from_numpy(_periodic(obs, B, 0)))
    p1 = np.ones((T, nb), np.float32) if pres is None else pres
    # the oracle's sequential accumulation in float32 (bits), per step
    canvas = np.zeros((nb, H, W), np.float32)
    if case.get("canvas_in"):
        canvas = _signed(rng, nb, H, W)
        d["canvas_in"] = Win((B, H, W))
        d["canvas_in"].v.copy_(torch.from_numpy(_periodic(canvas, B, 0)))
    steps = []
    for t in range(T):
        canvas = canvas + p1[t][:, None, None] * C.st_write_fwd(np.ascontiguousarray(glm[t]), np.ascontiguousarray(wh[t, :nb]), (H, W))
        steps.append(canvas.copy())
    d["steps32"], d["final32"] = np.stack(steps), steps[-1]
    if case.get("identity") and case["group"] == "X":
        return d
    # float64: every unit's write, the reconstruction term, dcanvas and the magnitudes of its summands
    K = T * nb
    ax, bx = axis_ab(wh[:, :nb].reshape(K, 4), "write", 0)
    ay, by = axis_ab(wh[:, :nb].reshape(K, 4), "write", 1)
    zero = np.zeros((K, H, W))
    fw = warp64(glm.reshape(K, h, w).astype(np.float64), ax, bx, ay, by, W, H, zero)
    v = fw["out"].reshape(T, nb, H, W) * p1.astype(np.float64)[:, :, None, None]
    vabs = fw["S_out_coord"].reshape(T, nb, H, W) * np.abs(p1.astype(np.float64))[:, :, None, None]
    final64, cabs = v.sum(0), vabs.sum(0)
    if case.get("canvas_in"):
        final64 = final64 + d["canvas_in"].v[:nb].double().numpy()
    d.update(final64=final64, write64=fw["out"].reshape(T, nb, H, W))
    mult, std = float(np.float32(MULT)), float(np.float32(STD))
    z = (obs.astype(np.float64) - mult * final64) / std
    cst = 0.5 * np.log(2 * np.pi) + np.log(std)
    d["rec64_pix"] = 0.5 * z * z + cst
    zabs = (np.abs(obs) + mult * cabs) / std
    d["S_rec_pix"] = z * z + np.abs(z) * zabs + abs(cst)
    if case["group"] == "X":
        return d
    loss_scale = 1.0 / B
    if case["entry"] == "write_bwd":
        dc = _signed(rng, nb, H, W)
        d["dcanvas"] = Win((B, H, W), "dcanvas" in off)
        d["dcanvas"].v.copy_(torch.from_numpy(_periodic(dc, B, 0)))
        dc64, dcabs = dc.astype(np.float64)[None], np.abs(dc).astype(np.float64)[None]
    else:
        # dcanvas of the final canvas the launch is GIVEN (stored form) or re-forms with the forward's own calls (recompute, fused): the
        # oracle's float32 accumulation, which group X holds the forward to bit for bit -- the backward is a function of that operand
        coef = loss_scale * mult / (std * std)
        f32c = d["final32"].astype(np.float64)
        dc64 = (coef * (mult * f32c - obs))[None]
        dcabs = (coef * (mult * np.abs(f32c) + np.abs(obs)))[None]
    d.update(loss_scale=loss_scale, dc64=dc64, dcabs=dcabs)
    bw = write_bwd64(glm.reshape(K, h, w), wh[:, :nb].reshape(K, 4), p1.reshape(K), np.broadcast_to(dc64, (T, nb, H, W)).reshape(K, H, W),
                     np.broadcast_to(dcabs, (T, nb, H, W)).reshape(K, H, W))
    for key in ("dglimpse", "dwhere", "dpresence"):
        shp = {"dglimpse": (T, nb, h, w), "dwhere": (T, nb, 4), "dpresence": (T, nb)}[key]
        d["an_" + key], d["S_" + key], d["P_" + key] = bw[key].reshape(shp), bw["S_" + key].reshape(shp), bw["P_" + key].reshape(shp)
    if case.get("identity"):                                # every coordinate an integer: the FLOAT32 scalar oracle is the reference
        # (per unit: the scalar loops on the step's glimpse with dout = p_t * dcanvas, both linear in dout; dpresence from their forward)
        dc32 = np.broadcast_to(dc64, (T, nb, H, W)).astype(np.float32)
        per = [C.st_write_bwd(np.ascontiguousarray(glm[t]), np.ascontiguousarray(wh[t, :nb]), p1[t][:, None, None] * dc32[t]) for t in range(T)]
        w32 = np.stack([C.st_write_fwd(np.ascontiguousarray(glm[t]), np.ascontiguousarray(wh[t, :nb]), (H, W)) for t in range(T)])
        d.update(dglimpse32=np.stack([x[0] for x in per]), dwhere32=np.stack([x[1] for x in per]),
                 dpresence32=(dc32.astype(np.float64) * w32).sum((2, 3)))
        return d
    ref = autograd_write(d, torch.float64)
    d.update({k + "64": v_ for k, v_ in ref.items()})
    return d


def autograd_write(d, dtype):
    """dglimpse, dwhere, dpresence by autograd through oracle.air_oracle.st_write in `dtype` (float64: the reference; float32: the restatement)"""
    case = d["case"]
    T, B, H, W, h, w = case["dims"]
    nb = d["nb"]
    tg = torch.tensor(d["glm_ref"], dtype=dtype, requires_grad=True)
    tw = torch.tensor(d["where_ref"], dtype=dtype, requires_grad=True)
    p1 = np.ones((T, nb), np.float32) if d["pres_ref"] is None else d["pres_ref"]
    tp = torch.tensor(p1, dtype=dtype, requires_grad=True)
    writes = [tp[t][:, None, None] * O.st_write(tg[t], tw[t], (H, W)) for t in range(T)]
    if case["entry"] == "write_bwd":
        loss = (torch.tensor(d["dcanvas"].v[:nb].numpy(), dtype=dtype) * writes[0]).sum()
    else:
        loss = (torch.tensor(d["dc64"][0], dtype=dtype) * sum(writes)).sum()        # dcanvas of the given final canvas (see data)
    gg, gw, gp = torch.autograd.grad(loss, [tg, tw, tp])
    return dict(dglimpse=gg.double().numpy(), dwhere=gw.double().numpy(), dpresence=gp.double().numpy())


def operands(case):
    """name -> (shape, is_output) of every pointer the case's entry takes (None: the case passes NULL), in the entry's own terms"""
    grp, entry, null = case["group"], case["entry"], set(case.get("null", ()))
    ops = {}
    pos = lambda *xs: tuple(max(int(x), 1) for x in xs)         # (a refused row's non-positive dimension: the buffers exist all the same)
    if grp in "VW":
        n_img, R, H, W, h, w = case["dims"]
        n = int(round(n_img * R))
        H, W, h, w = pos(H, W, h, w)
        ops = {"img": ((n_img, H, W), False), "where": ((n, 4), False)}
        if grp == "V":
            ops["glimpse"] = ((n, h, w), True)
        else:
            ops.update(dglimpse=((n, h, w), False), dwhere=((n, 4), True), dimg=((n_img, H, W), True) if case.get("dimg") else None)
    else:
        T1, B, H, W, h, w = pos(*case["dims"])
        ops = {"glimpse": ((T1, B, h, w), False), "where": ((T1, B, 4), False),
               "presence": ((T1, B), False) if case.get("pres") else None}
        if entry == "write_fwd":
            ops.update(canvas_in=((B, H, W), False) if case.get("canvas_in") else None, final=((B, H, W), True))
        elif entry in ("unroll_fwd", "banded", "fused"):
            outs = case.get("outs", "both")
            nbands = 1 if entry == "unroll_fwd" else case["n_bands"]
            ops.update(obs=((B, H, W), False), steps=((T1, B, H, W), True) if outs in ("both", "steps") else None,
                       final=((B, H, W), True) if outs in ("both", "final") else None,
                       rec_parts=((nbands, B), True) if case.get("rec", entry == "fused") else None)
            if entry == "fused":
                ops.update(dglimpse=((T1, B, h, w), True), dwhere=((case["n_split"], T1, B, 4), True))
        elif entry == "write_bwd":
            ops.update(dcanvas=((B, H, W), False), dglimpse=((T1, B, h, w), True), dwhere=((T1, B, 4), True),
                       dpresence=((T1, B), True) if case.get("dp") else None)
        else:
            ops.update(obs=((B, H, W), False), final=((B, H, W), False) if case["variant"] == "stored" else None,
                       dglimpse=((T1, B, h, w), True), dwhere=((T1, B, 4), True),
                       dpresence=((T1, B), True) if entry == "unroll_bwd_dp" else None)
    for k in null:
        ops[k] = None
    return ops


def query(case, addr):
    """the case's form query: addr(name) -> the operand's address or None.  -> (status, form dict)"""
    from attend_infer_repeat_amd import hip
    grp, entry = case["group"], case["entry"]
    if grp in "VW":
        n_img, R, H, W, h, w = case["dims"]
        n = int(round(n_img * R))
        if grp == "V":
            return hip.st_read_form(addr("img"), addr("where"), addr("glimpse"), n, n_img, H, W, h, w)
        return hip.st_read_bwd_form(addr("img"), addr("where"), addr("dglimpse"), addr("dwhere"), addr("dimg"), n, n_img, H, W, h, w)
    T, B, H, W, h, w = case["dims"]
    if entry == "write_fwd":
        return hip.canvas_fwd_form(addr("glimpse"), addr("where"), None, None, addr("final"), None, 1, 1, B, H, W, h, w)
    if entry in ("unroll_fwd", "banded"):
        return hip.canvas_fwd_form(addr("glimpse"), addr("where"), addr("obs"), addr("steps"), addr("final"), addr("rec_parts"),
                                   0 if entry == "unroll_fwd" else case["n_bands"], T, B, H, W, h, w)
    if entry == "fused":
        return hip.canvas_fwd_bwd_form(addr("glimpse"), addr("where"), addr("obs"), addr("steps"), addr("final"), addr("rec_parts"),
                                       case["n_bands"], addr("dglimpse"), addr("dwhere"), case["n_split"], T, B, H, W, h, w)
    if entry == "write_bwd":
        return hip.canvas_bwd_form(addr("glimpse"), addr("where"), addr("dcanvas"), None, None, addr("dglimpse"), addr("dwhere"), 1, B, H, W, h, w)
    if entry == "unroll_bwd_dp" and addr("dpresence") is None:
        return E_NULL, {}                                   # (the entry's own requirement, in front of the shared form function)
    return hip.canvas_bwd_form(addr("glimpse"), addr("where"), None, addr("final"), addr("obs"), addr("dglimpse"), addr("dwhere"),
                               T, B, H, W, h, w)


def host_addr(case):
    """fake addresses for the host test: aligned far beyond 16 bytes, 4 bytes further for the operands of `off`"""
    ops, off = operands(case), set(case["off"])
    return lambda name: None if ops.get(name) is None else Win.BASE + (4 if name in off else 0)


def bound(group, S):
    return CONST[group] * U32 * np.asarray(S, np.float64)


def rec_bound(S_pix_sum):
    return CONST["X"] * U32 * np.asarray(S_pix_sum, np.float64)
