"""Plain float64 restatement of the destriping cost and gradient (reference src/pyimcom/imdestripe.py: make_interpolated 476-594,
cost_function_single 1546-1559, residual_function_single 1375-1403, residual_function 1311-1317, transpose_par 1026-1058, the cost
models 875-902, compute_boundary_continuity_penalty 1413-1489) and of the two interpolation routines the reference takes from
furry_parakeet, under the cell rule its own tests state: coords are (y, x), the cell is floor, a target pixel whose cell is not wholly
inside the source contributes nothing.  tests/test_destripe_host.py pins it to the golden file's float64 run."""

import numpy as np


def _cells(coords, rows, cols):
    y, x = coords[:, 0], coords[:, 1]
    with np.errstate(invalid="ignore"):
        x1, y1 = np.floor(x), np.floor(y)
        ok = (x1 >= 0) & (y1 >= 0) & (x1 + 1 < cols) & (y1 + 1 < rows)
    idx = np.nonzero(ok)[0]
    x1, y1 = x1[idx].astype(np.int64), y1[idx].astype(np.int64)
    return idx, x1, y1, x[idx] - x1, y[idx] - y1


def bilinear_interpolation(image, g_eff, coords, out):
    """out (flat, += in place) the bilinear value of image * g_eff at coords [(y, x)]."""
    rows, cols = image.shape
    idx, x1, y1, dx, dy = _cells(np.asarray(coords, dtype=np.float64), rows, cols)
    src = image * g_eff
    val = ((1.0 - dx) * (1.0 - dy) * src[y1, x1] + dx * (1.0 - dy) * src[y1, x1 + 1] + (1.0 - dx) * dy * src[y1 + 1, x1] + dx * dy * src[y1 + 1, x1 + 1])
    flat = out.reshape(-1)
    flat[idx] += val.astype(out.dtype)


def bilinear_transpose(image, coords, out):
    """out [rows, cols] (+= in place): the transpose of the above applied to image (flat order of coords)."""
    rows, cols = out.shape
    idx, x1, y1, dx, dy = _cells(np.asarray(coords, dtype=np.float64), rows, cols)
    v = np.asarray(image).reshape(-1)[idx]
    acc = np.zeros((rows, cols), dtype=np.float64)
    np.add.at(acc, (y1, x1), (1.0 - dx) * (1.0 - dy) * v)
    np.add.at(acc, (y1, x1 + 1), dx * (1.0 - dy) * v)
    np.add.at(acc, (y1 + 1, x1), (1.0 - dx) * dy * v)
    np.add.at(acc, (y1 + 1, x1 + 1), dx * dy * v)
    out += acc.astype(out.dtype)


def f_cost(x, model, d=None):
    if model == "quadratic":
        return x ** 2
    if model == "absolute":
        return np.abs(x)
    return np.where(np.abs(x) <= d, x ** 2, d ** 2 + 2 * d * (np.abs(x) - d))


def f_prime(x, model, d=None):
    if model == "quadratic":
        return 2 * x
    if model == "absolute":
        return np.sign(x)
    return np.where(np.abs(x) <= d, 2 * x, 2 * d * np.sign(x))


def forward_par(params, nside, amp_cols):
    img = params[:nside, None] * np.ones((nside, nside))
    if amp_cols:
        img = img + np.repeat(params[nside:], amp_cols)[None, :]
    return img


def transpose_par(img, amp_cols):
    rows = np.sum(img, axis=1)
    if not amp_cols:
        return rows
    ncb = img.shape[1] // amp_cols
    return np.concatenate([rows, [np.sum(img[:, b * amp_cols:(b + 1) * amp_cols]) for b in range(ncb)]])


def penalty(img, mask, amp_cols, lam, cw=50, ch=100):
    n_rows, n_cols = img.shape
    pen = 0.0
    for b in range(1, n_cols // amp_cols):
        for r0 in range(0, n_rows, 4 * ch):
            rs = slice(r0, min(r0 + ch, n_rows))
            left, right = slice(b * amp_cols - cw, b * amp_cols), slice(b * amp_cols, b * amp_cols + cw)
            pen += (np.mean(img[rs, left][mask[rs, left]]) - np.mean(img[rs, right][mask[rs, right]])) ** 2
    return lam * pen


class Mosaic:
    """images float32, masks bool, g_eff float32 [n_sca, nside, nside]; coords[(a, b)] = (x_target, y_target) of a's pixels in b."""

    def __init__(self, images, masks, g_eff, coords, amp_cols=0, col_boundary_const=0.0, N_eff_min=0.5, psi_dtype=np.float64):
        self.img = np.asarray(images, dtype=np.float64)
        self.mask = np.asarray(masks, dtype=bool)
        self.g = np.asarray(g_eff, dtype=np.float64)
        self.n, self.nside = self.img.shape[0], self.img.shape[1]
        self.amp_cols, self.lam, self.nmin, self.psi_dtype = int(amp_cols or 0), float(col_boundary_const), float(N_eff_min), psi_dtype
        self.coords = {k: np.column_stack((np.ravel(v[1]), np.ravel(v[0]))).astype(np.float64) for k, v in coords.items()}
        self.nb = {a: sorted(b for (aa, b) in self.coords if aa == a) for a in range(self.n)}
        self.nbins = self.nside + (self.nside // self.amp_cols if self.amp_cols else 0)
        self.neff = np.zeros_like(self.img)
        for a in range(self.n):
            for b in self.nb[a]:
                tmp = np.zeros((self.nside, self.nside))
                bilinear_interpolation(self.mask[b].astype(np.float64), np.ones((self.nside, self.nside)), self.coords[(a, b)], tmp)
                self.neff[a] += tmp

    def destriped(self, params, k):
        v = self.img[k] - forward_par(params[k], self.nside, self.amp_cols)
        return np.where(np.isnan(v), 0, v * self.mask[k])

    def cost(self, params, model="quadratic", thresh=None):
        params = np.asarray(params, dtype=np.float64).reshape(self.n, self.nbins)
        psi = np.zeros((self.n, self.nside, self.nside), dtype=self.psi_dtype)
        eps = 0.0
        for a in range(self.n):
            ia = self.destriped(params, a)
            J = np.zeros((self.nside, self.nside))
            for b in self.nb[a]:
                tmp = np.zeros((self.nside, self.nside))
                bilinear_interpolation(self.destriped(params, b), self.g[b], self.coords[(a, b)], tmp)
                J += tmp
            nm = self.neff[a] > self.nmin
            with np.errstate(divide="ignore", invalid="ignore"):
                J = np.where(nm, J / np.where(nm, self.neff[a], self.nmin), 0)
                J = np.divide(J, self.g[a])
                psi[a] = np.where(nm * self.mask[a], ia - J, 0).astype(self.psi_dtype)
            local = np.sum(f_cost(psi[a].astype(np.float64), model, thresh))
            if self.amp_cols and self.lam > 0:
                local += penalty(ia, self.mask[a], self.amp_cols, self.lam)
            eps += local
        return eps, psi

    def residual(self, psi, model="quadratic", thresh=None, extrareturn=False):
        r = np.zeros((self.n, self.nbins))
        r1, r2 = np.zeros_like(r), np.zeros_like(r)
        for a in range(self.n):
            g = f_prime(np.asarray(psi[a], dtype=np.float64), model, thresh)
            t1 = transpose_par(g, self.amp_cols)
            r[a] -= t1
            r1[a] -= t1
            valid = self.neff[a] != 0
            with np.errstate(divide="ignore", invalid="ignore"):
                g = np.where(valid, g / (self.g[a] * self.neff[a]), 0)
            for b in self.nb[a]:
                go = np.zeros((self.nside, self.nside))
                bilinear_transpose(g, self.coords[(a, b)], go)
                go *= self.g[b]
                t2 = transpose_par(go, self.amp_cols)
                r[b] += t2
                r2[b] += t2
        return (r, r1, r2) if extrareturn else r

    # the reference's two signatures, for its optimiser
    def cost_function(self, p, f, thresh, workers, scalist, neighbors, cfg, tempdir=None, of=None, indata_type="fits"):
        eps, psi = self.cost(p.params, f.__name__ if f.__name__ != "huber_loss" else "huber", thresh)
        return eps, psi

    def residual_function(self, psi, fp, scalist, wcslist, neighbors, thresh, workers, cfg, extrareturn=False, of=None, indata_type="fits"):
        name = {"quad_prime": "quadratic", "abs_prime": "absolute", "huber_prime": "huber"}[fp.__name__]
        return self.residual(psi, name, thresh, extrareturn)


def poly_coords(coef, nside):
    """(x_target, y_target) [nside, nside] of a polynomial map with cubic terms: coef [2, 10] over the monomials u^i v^j, i + j <= 3, of
    u = x / nside - 1/2, v = y / nside - 1/2 (in the order i = 0 .. 3, j = 0 .. 3 - i)."""
    y, x = np.meshgrid(np.arange(nside, dtype=np.float64), np.arange(nside, dtype=np.float64), indexing="ij")
    u, v = x / nside - 0.5, y / nside - 0.5
    mono = [u ** i * v ** j for i in range(4) for j in range(4 - i)]
    return tuple(sum(c * m for c, m in zip(coef[k], mono)) for k in range(2))


def synthetic_maps(n_sca, nside, seed, roll_deg=(3.0, -7.0, 12.0, 40.0), cubic=0.4):
    """coef[(a, b)] for every ordered pair: b's frame is a's rolled by the difference of their roll angles about the centre, shifted
    by up to a third of a side, bent by quadratic and cubic terms of `cubic` pixels."""
    rng = np.random.default_rng(seed)
    out = {}
    for a in range(n_sca):
        for b in range(n_sca):
            if a == b:
                continue
            th = np.deg2rad(roll_deg[b % len(roll_deg)] - roll_deg[a % len(roll_deg)])
            sh = rng.uniform(-nside / 3.0, nside / 3.0, size=2)
            coef = rng.uniform(-cubic, cubic, size=(2, 10))
            c, s = np.cos(th) * nside, np.sin(th) * nside
            # monomial order: (0,0) (0,1) (0,2) (0,3) (1,0) (1,1) (1,2) (2,0) (2,1) (3,0)
            coef[0, 0], coef[0, 4], coef[0, 1] = (nside - 1) / 2.0 + sh[0] + 0.2371, c, -s
            coef[1, 0], coef[1, 4], coef[1, 1] = (nside - 1) / 2.0 + sh[1] + 0.4113, s, c
            out[(a, b)] = coef
    return out


def replay_line_searches(cost_function, residual_function, points, f, f_prime, scalist, neighbors):
    """Replay a recorded run of an optimiser over the two bound functions.  ``points`` [1 + 2 k, n_sca, nbins] are the parameter vectors
    the recorded run evaluated the cost at: the start, then per line search a probe point and the point it settled on.  The calls are made
    in the recorded order -- cost at the start and its gradient; per line search cost and gradient at the probe (that psi dropped), cost
    at the settled point -- and every psi goes back to ``residual_function`` as the very array ``cost_function`` returned.

    From the gradients that come back the settled points are formed again, in this project's terms: the cost is a quadratic form, so
    along the segment v = probe - x its gradient is linear, and with g0 at x and g1 at the probe the minimum lies at
    x + lam v, lam = -(v . g0) / (v . (g1 - g0)); the gradient there is g0 + lam (g1 - g0) and serves as g0 of the next search.
    Returns {"eps": [...], "resids": [...], "settled": [...]} in call order."""
    import types

    out = {"eps": [], "resids": [], "settled": []}
    n = len(scalist)

    def evaluate(x, want_gradient):
        eps, psi = cost_function(types.SimpleNamespace(params=np.array(x)), f, None, 1, scalist, neighbors, None)
        out["eps"].append(eps)
        if want_gradient:
            out["resids"].append(residual_function(psi, f_prime, scalist, [None] * n, neighbors, None, 1, None))
        del psi
        return out["resids"][-1] if want_gradient else None

    g0 = evaluate(points[0], True)
    for k in range((len(points) - 1) // 2):
        x, probe = points[2 * k], points[2 * k + 1]
        g1 = evaluate(probe, True)
        v = probe - x
        lam = -np.vdot(v, g0) / np.vdot(v, g1 - g0)
        out["settled"].append(x + lam * v)
        g0 = g0 + lam * (g1 - g0)
        evaluate(points[2 * k + 2], False)
    return out
