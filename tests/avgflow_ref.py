"""TEST INFRASTRUCTURE: the reference of the average-flow alignment of a slice list (CLI
"style": 2; tvl1_blend6_u8, tvl1_half_u8, tvl1_remap_flow_u8).

A numpy restatement of the arithmetic, stage by stage:

  weights()   float(float(exp(-d^2 / 4)) * s), d = 3, 2, 1, s = 0.5 / (e3 + e2 + e1) in double,
              mirrored: the six neighbours i-3 .. i+3 without i;
  blend6      a double accumulator over the six u8 frames, rounded half-to-even, saturated;
  half        (a + b + c + d + 2) >> 2 over 2x2 blocks (cv::resize of u8 at exactly 1/2);
  flow_up     g(t) = float(double(t) * gain) on every tap, then cv::resize INTER_LINEAR with
              half-pixel centres to the frame's size, operation for operation as the engine's
              k_resize_hp bilinear branch (float32 products and sums, no fma);
  remap       canvas px (X, Y) -> frame coordinate (x, y) = (X - b, Y - b), the flow of the
              nearest frame px, the map (x - U, y - V) rounded to 1/32 px (rint; INT_MIN for
              NaN or out of range), coordinates saturated to short, four taps checked against
              the frame one by one (outside: 0), 5-bit weights, (sum + 512) >> 10;
  align_slice blend -> pre-scale -> oracle.checker.oracle_calc -> remap.

Also here: the slice stacks of the GPU end-to-end cases, so the CPU suite can hold every solve
they make to the project's residual margin, and a cache so each reference is computed once."""
from __future__ import annotations

import numpy as np

from optflow_amd import capi, synth
from oracle import checker

INT_MIN = -2 ** 31


def weights() -> np.ndarray:
    e = np.exp(np.array([-9.0 / 4.0, -1.0, -1.0 / 4.0], np.float64))
    s = 0.5 / (e[0] + e[1] + e[2])
    w = (e.astype(np.float32).astype(np.float64) * s).astype(np.float32)
    return np.array([w[0], w[1], w[2], w[2], w[1], w[0]], np.float32)


def blend6(frames, order=range(6)) -> np.ndarray:
    """frames: the six neighbours (i-3, i-2, i-1, i+1, i+2, i+3); order: the summation order
    (the sum is exact in double, so any order gives the same bits)."""
    w = weights().astype(np.float64)
    acc = np.zeros(np.asarray(frames[0]).shape, np.float64)
    for k in order:
        acc = acc + w[k] * np.asarray(frames[k], np.uint8).astype(np.float64)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def half(a) -> np.ndarray:
    a = np.asarray(a, np.uint8).astype(np.int32)
    assert a.shape[0] % 2 == 0 and a.shape[1] % 2 == 0
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def _axis(n_dst, n_src):
    """Per destination index: source index, fraction and single-tap flag along x, and the two
    clamped rows with their weights along y (k_resize_hp's bilinear branch)."""
    scale = float(n_src) / float(n_dst)
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = (f - s.astype(np.float32)).astype(np.float32)
    return s, f


def flow_up(f, W, H, gain) -> np.ndarray:
    """One flow component at every frame px: float32 (H, W)."""
    f = np.asarray(f, np.float32)
    fh, fw = f.shape
    with np.errstate(all="ignore"):
        g = (f.astype(np.float64) * float(gain)).astype(np.float32)
        if (fw, fh) == (W, H):
            return g
        sy, fy = _axis(H, fh)
        b0, b1 = (np.float32(1) - fy).astype(np.float32), fy
        r0, r1 = np.clip(sy, 0, fh - 1), np.clip(sy + 1, 0, fh - 1)
        sx, fx = _axis(W, fw)
        neg = sx < 0
        fx[neg], sx[neg] = 0, 0
        single = sx + 1 >= fw
        last = sx >= fw - 1
        fx[last], sx[last] = 0, fw - 1
        a0, a1 = (np.float32(1) - fx).astype(np.float32), fx
        sx1 = np.minimum(sx + 1, fw - 1)
        one = np.float32(1)

        def row(S):
            two = S[:, sx] * a0[None, :] + S[:, sx1] * a1[None, :]
            return np.where(single[None, :], S[:, sx] * one, two).astype(np.float32)

        t0, t1 = row(g[r0]), row(g[r1])
        return (t0 * b0[:, None] + t1 * b1[:, None]).astype(np.float32)


def round_map(v) -> np.ndarray:
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        ok = (v > np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))
        r = np.where(ok, np.rint(v), 0).astype(np.int64)
    r[~ok] = INT_MIN
    return r.astype(np.int32)


def remap(frame, u, v, gain=1.0, border=0) -> np.ndarray:
    frame = np.asarray(frame, np.uint8)
    H, W = frame.shape
    b = int(border)
    U, V = flow_up(u, W, H, gain), flow_up(v, W, H, gain)
    X = np.arange(W + 2 * b, dtype=np.int32) - b
    Y = np.arange(H + 2 * b, dtype=np.int32) - b
    xc, yc = np.clip(X, 0, W - 1), np.clip(Y, 0, H - 1)
    with np.errstate(all="ignore"):
        mx = (X.astype(np.float32)[None, :] - U[yc][:, xc]).astype(np.float32)
        my = (Y.astype(np.float32)[:, None] - V[yc][:, xc]).astype(np.float32)
        ix, iy = round_map(mx * np.float32(32)), round_map(my * np.float32(32))
    sx, fx = np.clip(ix >> 5, -32768, 32767), ix & 31
    sy, fy = np.clip(iy >> 5, -32768, 32767), iy & 31
    fr = frame.astype(np.int32)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(ok, fr[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0)

    s = (tap(sy, sx) * (32 - fx) * (32 - fy) + tap(sy, sx + 1) * fx * (32 - fy) +
         tap(sy + 1, sx) * (32 - fx) * fy + tap(sy + 1, sx + 1) * fx * fy + 512) >> 10
    return s.astype(np.uint8)


def prescale_path(W, H, scale) -> str:
    if scale == 1:
        return "none"
    return "device" if scale == 0.5 and W % 2 == 0 and H % 2 == 0 else "host"


def align_slice(frames7, params=None, scale=0.5, border=0, prescaled=None):
    """frames7: slices i-3 .. i+3.  prescaled = (I0, I1): the pre-scaled slice and blend of a
    job on the host path (made by the CLI's own --decode hook, not restated here).  Returns
    (aligned, u, v, warp_iters, stats, (I0, I1))."""
    F = np.asarray(frames7[3], np.uint8)
    B = blend6(list(frames7[:3]) + list(frames7[4:]))
    H, W = F.shape
    path = prescale_path(W, H, scale)
    if prescaled is not None:
        I0, I1 = prescaled
    elif path == "none":
        I0, I1 = F, B
    elif path == "device":
        I0, I1 = half(F), half(B)
    else:
        raise ValueError("a host pre-scale needs the pre-scaled pair")
    u, v, st, wi = checker.oracle_calc(I0, I1, params or capi.make_params())
    return remap(F, u, v, 1.0 / scale, border), u, v, wi, st, (I0, I1)


# ---- the end-to-end cases of the GPU tests (tests/test_gpu_avgflow.py, test_cli_avgflow_gpu.py)
# name -> width, height, slices, rng seed, scale, border, TV-L1 keys (JSON names).  The seeds
# were chosen on the CPU so that every solve clears MIN_MARGIN (test_avgflow_ref_cpu.py).
TV = dict(nscales=4, warps=3)
STACKS = {
    "half_96x64": dict(w=96, h=64, n=9, seed=2, scale=0.5, border=4),
    "full_80x48": dict(w=80, h=48, n=7, seed=3, scale=1.0, border=4),
    "host_67x45": dict(w=67, h=45, n=9, seed=4, scale=0.5, border=4),
}
_cache: dict = {}


def stack_of(name) -> np.ndarray:
    c = STACKS[name]
    key = ("stack", name)
    if key not in _cache:
        _cache[key] = synth.gen_stack(c["w"], c["h"], c["n"], seed=c["seed"])
    return _cache[key]


def outputs_of(name):
    return list(range(3, STACKS[name]["n"] - 3))


def reference(name, i, prescaled=None):
    """align_slice of output i of a stack, computed once."""
    key = ("ref", name, i)
    if key not in _cache:
        c, st = STACKS[name], stack_of(name)
        _cache[key] = align_slice([st[k] for k in range(i - 3, i + 4)], capi.make_params(**TV),
                                  c["scale"], c["border"], prescaled)
    return _cache[key]


def tie_frames(count=16):
    """Six frames of `count` px whose weighted sums are exact .5 ties, found by a directed
    search: with the mirrored weights, sum = w0 (a0 + a5) + w1 (a1 + a4) + w2 (a2 + a3), so
    it is enough to search the pair sums p, q, r in [0, 510] for w0 p + w1 q + w2 r = k + 1/2
    in units of 2^-28.  Returns (frames (6, count) u8, floors k), both parities of k present."""
    w = weights().astype(np.float64) * 2.0 ** 28
    w0, w1, w2 = (int(w[0]), int(w[1]), int(w[2]))
    assert (w0, w1, w2) == tuple(w[:3])
    one, found = 1 << 28, {0: [], 1: []}
    p = np.arange(511, dtype=np.int64)
    for r in range(511):
        tot = w0 * p[:, None] + w1 * p[None, :] + w2 * r
        hit = np.argwhere(tot % one == one // 2)
        for a, b in hit:
            k = int(tot[a, b] // one)
            if len(found[k & 1]) < count // 2:
                found[k & 1].append((int(a), int(b), r, k))
        if all(len(v) >= count // 2 for v in found.values()):
            break
    sel = found[0] + found[1]
    fr = np.zeros((6, len(sel)), np.uint8)
    for j, (a, b, r, _) in enumerate(sel):
        for lo, hi, s in ((0, 5, a), (1, 4, b), (2, 3, r)):
            fr[lo, j], fr[hi, j] = s // 2, s - s // 2
    return fr, np.array([k for *_, k in sel])
