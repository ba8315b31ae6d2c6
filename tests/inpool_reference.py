"""Reference for the input-stamp pool (seam 17), independent of pyimcom_amd: a vectorised numpy restatement of the reference's sparse-grid
relevance test (src/pyimcom/coadd.py:206-233), of the binning loop of InImage.partition_pixels (329-358), of InImage.extract_layers (394-404)
and of InStamp.__init__ (688-707).  Every function takes the POSITIONS as an argument -- where they come from (numpy's WCS chain for the golden
file, the device's for the GPU tests) is the caller's business; given the same positions the results are the reference's, element for element
(tests/test_inpool_host.py holds them to tests/golden/inpool.npz, which the reference's own statements wrote)."""

import numpy as np


def frames(n_inframe, nside, image_no=0):
    """Input layers [n_inframe, nside, nside] float32 whose every value names its own (image, frame, y, x) exactly (nside <= 256)."""
    assert nside <= 256 and (image_no * 4 + n_inframe) * 65536 < 2 ** 24
    f, y, x = np.meshgrid(np.arange(n_inframe), np.arange(nside), np.arange(nside), indexing="ij")
    return ((image_no * 4 + f) * 65536 + y * 256 + x).astype(np.float32)


def limits(n2, n1P):
    """(pix_lower, pix_upper) of coadd.py:207-208, NsideP = n1P n2."""
    return -n2 - 0.5, n1P * n2 + n2 - 0.5


def sparse_axis(nside, sp_res):
    return np.linspace(0, nside, sp_res + 1, dtype=np.uint16)


def relevance(sp_outxys, use_instamps, n2, n1P):
    """(is_relevant, relevant_matrix [sp_res, sp_res]) from the node positions sp_outxys [2, sp_res + 1, sp_res + 1] (x plane, y plane)."""
    sp_res = sp_outxys.shape[1] - 1
    lo, hi = limits(n2, n1P)
    nst = n1P + 2
    x, y = sp_outxys[0, 1:sp_res, 1:sp_res], sp_outxys[1, 1:sp_res, 1:sp_res]  # the interior nodes
    with np.errstate(invalid="ignore"):
        inr = (lo < x) & (x < hi) & (lo < y) & (y < hi)
    jj, ii = np.nonzero(inr)
    ist = ((x[jj, ii] - lo) // n2).astype(int)
    jst = ((y[jj, ii] - lo) // n2).astype(int)
    # any use_instamps in the clipped 5 x 5 window: a 2-D inclusive prefix sum
    cum = np.zeros((nst + 1, nst + 1), dtype=np.int64)
    cum[1:, 1:] = np.cumsum(np.cumsum(np.asarray(use_instamps, dtype=np.int64), axis=0), axis=1)
    j0, j1, i0, i1 = np.maximum(jst - 2, 0), np.minimum(jst + 3, nst), np.maximum(ist - 2, 0), np.minimum(ist + 3, nst)
    hit = (cum[j1, i1] - cum[j0, i1] - cum[j1, i0] + cum[j0, i0]) > 0
    hit &= (j1 > j0) & (i1 > i0)
    matrix = np.zeros((sp_res, sp_res), dtype=bool)
    for j, i in zip(jj[hit] + 1, ii[hit] + 1):
        matrix[max(j - 2, 0):min(j + 3, sp_res), max(i - 2, 0):min(i + 3, sp_res)] = True
    return bool(hit.any()), matrix


def visits(relevant, sp_arr):
    """(y, x) int arrays of the visited pixels in visiting order."""
    sp = np.asarray(sp_arr).astype(np.int64)
    ys, xs = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for j, i in zip(*np.nonzero(relevant)):
        h, w = sp[j + 1] - sp[j], sp[i + 1] - sp[i]
        ys.append(np.repeat(np.arange(sp[j], sp[j + 1]), w))
        xs.append(np.tile(np.arange(sp[i], sp[i + 1]), h))
    return np.concatenate(ys), np.concatenate(xs)


class Overflow(Exception):
    pass


def partition(pos_x, pos_y, relevant, sp_arr, mask, use_instamps, n2, n1P, npixmax):
    """pos_x, pos_y [nside, nside]: the block position of every input pixel (NaN allowed).  Returns y_idx, x_idx (uint16), y_val, x_val (float64)
    [nst, nst, npixmax] and pix_count (uint32) [nst, nst]; Overflow where the reference would index past npixmax."""
    nst = n1P + 2
    lo, hi = limits(n2, n1P)
    vy, vx = visits(relevant, sp_arr)
    x, y = pos_x[vy, vx], pos_y[vy, vx]
    with np.errstate(invalid="ignore"):
        keep = (lo < x) & (x < hi) & (lo < y) & (y < hi)
    if mask is not None:
        keep &= np.asarray(mask, dtype=bool)[vy, vx]
    at = np.nonzero(keep)[0]
    ist, jst = ((x[at] - lo) // n2).astype(int), ((y[at] - lo) // n2).astype(int)
    used = np.asarray(use_instamps, dtype=bool)[jst, ist]
    at, key = at[used], (jst * nst + ist)[used]
    order = np.argsort(key, kind="stable")
    at, key = at[order], key[order]
    count = np.bincount(key, minlength=nst * nst)
    if count.max(initial=0) > npixmax:
        raise Overflow(int(count.max()))
    slot = np.arange(len(key)) - (np.cumsum(count) - count)[key]
    y_idx, x_idx = np.zeros((nst * nst, npixmax), np.uint16), np.zeros((nst * nst, npixmax), np.uint16)
    y_val, x_val = np.zeros((nst * nst, npixmax)), np.zeros((nst * nst, npixmax))
    y_idx[key, slot], x_idx[key, slot], y_val[key, slot], x_val[key, slot] = vy[at], vx[at], y[at], x[at]
    shape = (nst, nst, npixmax)
    return y_idx.reshape(shape), x_idx.reshape(shape), y_val.reshape(shape), x_val.reshape(shape), count.astype(np.uint32).reshape(nst, nst)


def extract_layers(indata, y_idx, x_idx, pix_count, max_count=None):
    """data [n_inframe, nst, nst, max_count] float32."""
    max_count = int(pix_count.max()) if max_count is None else int(max_count)
    on = np.arange(max_count) < pix_count[..., None]
    data = indata[:, y_idx[..., :max_count], x_idx[..., :max_count]].astype(np.float32)
    return np.where(on[None], data, np.float32(0))


def instamps(images, n_inframe):
    """images: the relevant images in list order, each a dict with y_val, x_val, data, pix_count.  Returns (list over the stamps, row-major, of
    (x_val, y_val, data [n_inframe, k], pix_cumsum uint32 [n_img + 1]) -- the tuples select.InStampPool takes --, pix_cumsum [nst^2, n_img + 1])."""
    nst = images[0]["pix_count"].shape[0] if images else 0
    out = []
    for j in range(nst):
        for i in range(nst):
            cnt = [int(im["pix_count"][j, i]) for im in images]
            cum = np.cumsum([0] + cnt, dtype=np.uint32)
            xs = np.concatenate([im["x_val"][j, i, :c] for im, c in zip(images, cnt)])
            ys = np.concatenate([im["y_val"][j, i, :c] for im, c in zip(images, cnt)])
            ds = np.concatenate([im["data"][:n_inframe, j, i, :c] for im, c in zip(images, cnt)], axis=1)
            out.append((xs, ys, ds, cum))
    return out, np.array([t[3] for t in out], dtype=np.uint32).reshape(nst * nst, len(images) + 1)


def pool_arrays(stamps):
    """(x, y, data, expo, inst_off) of a list of InStamp tuples, as select.InStampPool lays them out."""
    off = np.concatenate([[0], np.cumsum([len(t[0]) for t in stamps])]).astype(np.int64)
    x, y = np.concatenate([t[0] for t in stamps]), np.concatenate([t[1] for t in stamps])
    data = np.concatenate([t[2] for t in stamps], axis=1)
    expo = np.concatenate([np.repeat(np.arange(len(t[3]) - 1), np.diff(t[3].astype(np.int64))) for t in stamps]).astype(np.int32)
    return x, y, data, expo, off
