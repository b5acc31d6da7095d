"""Plain NumPy restatement of the specular echo times of sampled reflectors (include/rtus.h: rtus_specular) and of the
one-parameter fit built on them (api.fit_reflector).  Vectorised over the pairs, sequential in meaning: every sum is one fp64
addition, the refinement is the header's sequence of single operations, so the kernel's results are these bits.  Nothing here touches
the GPU.  The oracle of tests/test_specular_cpu.py and tests/test_gpu_specular.py."""
import numpy as np


def specular(tt_a, tt_b=None, n_refl=1):
    """tt_a [n_a, n_refl n_p], tt_b [n_b, n_refl n_p] (None: tt_a) -> (t, pos float64, n_min int32), each [n_refl, n_a, n_b]"""
    A = np.asarray(tt_a, dtype=np.float64)
    B = A if tt_b is None else np.asarray(tt_b, dtype=np.float64)
    n_a, n_b, n_p = A.shape[0], B.shape[0], A.shape[1] // n_refl
    t = np.full((n_refl, n_a, n_b), np.nan)
    pos = np.full((n_refl, n_a, n_b), np.nan)
    n_min = np.zeros((n_refl, n_a, n_b), dtype=np.int32)
    for g in range(n_refl):
        cols = slice(g * n_p, (g + 1) * n_p)
        with np.errstate(all="ignore"):
            S = A[:, None, cols] + B[None, :, cols]                    # [n_a, n_b, n_p]
            fin = np.isfinite(S)
            if n_p >= 3:
                mid = S[..., 1:-1]
                n_min[g] = np.sum(fin[..., :-2] & fin[..., 1:-1] & fin[..., 2:] & (mid < S[..., :-2]) & (mid < S[..., 2:]), axis=-1)
            some = fin.any(axis=-1)
            js = np.argmin(np.where(fin, S, np.inf), axis=-1)          # the first index of the least finite sum
            pos[g] = np.where(some, js.astype(np.float64), np.nan)
            inner = some & (js > 0) & (js < n_p - 1)
            take = lambda d: np.take_along_axis(S, np.clip(js + d, 0, n_p - 1)[..., None], axis=-1)[..., 0]      # noqa: E731
            a, b, c = take(-1), take(0), take(1)
            ok = inner & np.isfinite(a) & np.isfinite(c)
            d1 = a - c
            d2 = (a - b) + (c - b)
            delta = 0.5 * d1 / d2
            t[g] = np.where(ok, b - (0.25 * d1) * delta, np.nan)
            pos[g] = np.where(ok, js + delta, pos[g])
    return t, pos, n_min


def misfit_stats(tt, t_meas, w=None, fit_delay=False):
    """-> (mse, n, delay) [G] over the pairs where both times are finite and the weight is positive (api._misfit_stats' formulas)"""
    tt, tm = np.asarray(tt, dtype=np.float64), np.asarray(t_meas, dtype=np.float64)
    wt = np.ones_like(tm) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = tt - tm[None]
        use = np.isfinite(r) & (wt > 0)[None]
        r = np.where(use, r, 0.0)
        wu = np.where(use, wt[None], 0.0)
        n = use.sum(axis=(1, 2))
        sse, sr, sw = (wu * r * r).sum(axis=(1, 2)), (wu * r).sum(axis=(1, 2)), wu.sum(axis=(1, 2))
        if fit_delay:
            return np.where(n > 0, np.maximum(sse - sr * sr / sw, 0.0) / n, np.nan), n, np.where(n > 0, -sr / sw, np.nan)
        return np.where(n > 0, sse / n, np.nan), n, np.where(n > 0, 0.0, np.nan)


def final_spacing(lo, hi, n_grid=33, passes=3):
    """the grid spacing of the last pass"""
    return (hi - lo) * (2.0 / (n_grid - 1)) ** (passes - 1) / (n_grid - 1)


def fit(t_meas, model, lo, hi, *, n_grid=33, passes=3, w=None, fit_delay=False, min_pairs=8):
    """api.fit_reflector's procedure: per pass n_grid values over the bracket, the first of least mse among those with min_pairs
    pairs, next bracket its two neighbours; then the parabola through the best and its neighbours, clamped to them."""
    def score(values):
        mse, n, delay = misfit_stats(model(values), t_meas, w, fit_delay)
        return np.where(n >= min_pairs, mse, np.nan), n, delay

    a, b, ok, history = float(lo), float(hi), True, []
    fail = dict(value=np.nan, mse=np.nan, n=0, delay=np.nan, ok=False, history=history)
    for it in range(passes):
        values = np.linspace(a, b, n_grid)
        mse, n, _ = score(values)
        if not np.isfinite(mse).any():
            return fail
        k = int(np.nanargmin(mse))
        history.append(dict(values=values, mse=mse, n=n, best=k))
        if it == 0 and k in (0, n_grid - 1):
            ok = False
        a, b = values[max(k - 1, 0)], values[min(k + 1, n_grid - 1)]
    value = values[k]
    if 0 < k < n_grid - 1 and np.isfinite(mse[k - 1]) and np.isfinite(mse[k + 1]):
        d2 = (mse[k - 1] - mse[k]) + (mse[k + 1] - mse[k])
        if d2 > 0:
            value = min(max(value + 0.5 * (mse[k - 1] - mse[k + 1]) / d2 * (values[k + 1] - values[k]), a), b)
    mse, n, delay = score(np.asarray([value]))
    if not np.isfinite(mse[0]):
        return fail
    return dict(value=float(value), mse=float(mse[0]), n=int(n[0]), delay=float(delay[0]), ok=ok, history=history)
