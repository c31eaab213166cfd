"""float64 numpy restatements of the two device augmentation stages, written from the maths (no reference code is imported here):
the thin-plate-spline warp in the reference's semantics, and torch's antialiased bilinear resized crop with a horizontal flip.
tests/golden/tps_warp.npz (made by tests/golden/make_golden_tps.py from the real reference) pins the first; torch's CPU interpolate the second."""
import numpy as np


def corners(W):
    return np.array([[0, 0], [0, W], [W, 0], [W, W]], dtype=np.float64)


def _U(r):
    with np.errstate(divide="ignore", invalid="ignore"):
        return r * r * np.where(r < 1e-100, 0.0, np.log(np.where(r < 1e-100, 1.0, r)))


def tps_L(P):
    """The (K + 3) x (K + 3) thin-plate system of the control points P [K, 2]."""
    K = len(P)
    d = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    L = np.zeros((K + 3, K + 3))
    L[:K, :K] = _U(d)
    L[:K, K] = 1.0
    L[:K, K + 1:] = P
    L[K, :K] = 1.0
    L[K + 1:, :K] = P.T
    return L


def tps_coefficients_ref(dst, src, W):
    """dst, src [k, 2] -> (P [k + 4, 2], coef [2, k + 7]): the spline that takes the displaced points (and the corners) back to the regular ones."""
    P = np.concatenate([np.asarray(dst, np.float64), corners(W)])
    V = np.zeros((len(P) + 3, 2))
    V[:len(P)] = np.concatenate([np.asarray(src, np.float64), corners(W)])
    return P, (np.linalg.pinv(tps_L(P)) @ V).T.copy()


def fold_reflect(i, W):
    """Half-sample symmetric extension (scipy's mode='reflect'): -1 -> 0, W -> W - 1, period 2 W."""
    m = np.mod(i, 2 * W)
    return np.where(m < W, m, 2 * W - 1 - m)


def tps_coords(P, coef, W):
    """The (axis-0, axis-1) sampling coordinates of every pixel, [2, W, W] float64."""
    steps = (W - 1) / 10
    n = int(steps)
    g = np.arange(n) * ((W - 1) / float(n - 1))
    gx, gy = np.meshgrid(g, g, indexing="ij")
    r = np.sqrt((P[:, 0] - gx[..., None]) ** 2 + (P[:, 1] - gy[..., None]) ** 2)
    u = _U(r)
    K = len(P)
    coarse = [coef[a, K] + coef[a, K + 1] * gx + coef[a, K + 2] * gy + (coef[a, :K] * u).sum(-1) for a in (0, 1)]
    pos = (steps - 1) * np.arange(W) / float(W - 1)
    idx = pos.astype(np.int64)
    fr = pos - idx
    up = np.minimum(idx + 1, int(steps - 1))
    xi, yi = idx[:, None], idx[None, :]
    xu, yu = up[:, None], up[None, :]
    xf, yf = fr[:, None], fr[None, :]
    out = []
    for t in coarse:
        out.append(t[xi, yi] * (1 - xf) * (1 - yf) + t[xi, yu] * (1 - xf) * yf + t[xu, yi] * xf * (1 - yf) + t[xu, yu] * xf * yf)
    return np.stack(out)


def sample_reflect(img, coords):
    """img [C, W, W], coords [2, W, W] -> bilinear samples with the reflect fold, float64."""
    W = img.shape[-1]
    img = img.astype(np.float64)
    f0 = np.floor(coords)
    t = coords - f0
    i0 = f0.astype(np.int64)
    a0, a1 = fold_reflect(i0[0], W), fold_reflect(i0[0] + 1, W)
    b0, b1 = fold_reflect(i0[1], W), fold_reflect(i0[1] + 1, W)
    tx, ty = t[0], t[1]
    return ((1 - tx) * ((1 - ty) * img[:, a0, b0] + ty * img[:, a0, b1]) + tx * ((1 - ty) * img[:, a1, b0] + ty * img[:, a1, b1]))


def tps_warp_ref(img, dst, src):
    """img [C, W, W] -> the reference's tps_warp_2 of it (channels first), float64."""
    W = img.shape[-1]
    P, coef = tps_coefficients_ref(dst, src, W)
    return sample_reflect(img, tps_coords(P, coef, W))


def aa_weights(n_in, S):
    """[S, n_in] float64 weights of torch's antialiased bilinear resize along one axis."""
    scale = n_in / S
    support = max(scale, 1.0)
    M = np.zeros((S, n_in))
    for o in range(S):
        center = scale * (o + 0.5)
        lo = max(0, int(center - support + 0.5))
        hi = min(n_in, int(center + support + 0.5))
        j = np.arange(lo, hi)
        w = np.maximum(0.0, 1.0 - np.abs((j - center + 0.5) / support))
        M[o, lo:hi] = w / w.sum()
    return M


def crop_resize_flip_ref(img, box, flip, S):
    """img [C, H, W], box (i, j, h, w) -> [C, S, S] float64."""
    i, j, h, w = (int(v) for v in box)
    out = aa_weights(h, S) @ img[:, i:i + h, j:j + w].astype(np.float64) @ aa_weights(w, S).T
    return out[:, :, ::-1] if flip else out


def tps_bound(img, W):
    """|out - ref| allowed for the fp32 warp: a coordinate error of W 2^-21 pixel times the bilinear slope on both axes, plus the blend's rounding."""
    x = img.astype(np.float64)
    G = max(np.abs(np.diff(x, axis=-1)).max(), np.abs(np.diff(x, axis=-2)).max())
    return 2 * G * W * 2.0 ** -21 + 4 * 2.0 ** -24 * np.abs(x).max()


def crop_bound(img, h, w):
    return 18 * max(h, w) * 2.0 ** -24 * np.abs(img.astype(np.float64)).max()
