"""numpy restatement of the coaddition stage of the reference's PSFSPLIT pipeline (reference src/pyimcom/psfutil.py), pinned to the
reference's own outputs by tests/test_psfsplit_host.py (tests/golden/psfsplit.npz) and used as the yardstick of tests/test_gpu_psfsplit.py.

Under ``PSFGrp.setup(..., psfsplit=True)`` two things differ from the unsplit pipeline the oracle restates (oracle/oracle.py):

* PSFOvl.setup 1087-1089: the overlap tables have the side ``2 * PSFGrp.nsamp + 1 = nfft - 1`` and the centre ``PSFGrp.nsamp``, while the
  PSFs keep their side.  The oracle's functions take their geometry as an object, so ``SplitGeom`` carries two: ``psf`` (for
  ``pad_and_rfft2``, sampling, targets) and ``tab`` (for ``overlap_*`` and the sub-block functions).
* PSFGrp._sample_psf 739-753: the sampling positions come from four evaluations of the pixel map (``cardinal_points``,
  ``affine_yxco``) instead of nsamp^2.
"""

import numpy as np

from oracle import oracle as orc


class _TableGeom:
    """PSFOvl's class attributes under psfsplit (psfutil.py:1087-1089) beside what the sub-block functions read from PSFGrp."""

    def __init__(self, psf):
        self.nsamp, self.nc = 2 * psf.nsamp + 1, psf.nsamp
        self.nfft, self.oversamp, self.dscale, self.flat_penalty = psf.nfft, psf.oversamp, psf.dscale, psf.flat_penalty


class SplitGeom:
    def __init__(self, npixpsf, oversamp, dtheta_deg, flat_penalty=1e-7):
        self.psf = orc.Geom(npixpsf, oversamp, dtheta_deg, flat_penalty)
        self.tab = _TableGeom(self.psf)
        assert self.tab.nsamp == self.psf.nfft - 1

    def set_flat_penalty(self, fp):
        self.psf.flat_penalty = self.tab.flat_penalty = fp


def cardinal_points(outpix2world2inpix, point, oversamp, dscale):
    """yx_cardinal of psfutil.py:739-749: [4, 2] (y, x)."""
    p = np.array(point)[None, :] + np.array([[1, 0], [0, 1], [-1, 0], [0, -1]]) * oversamp
    return np.flip(outpix2world2inpix(p), axis=-1) / 2.0 * dscale


def affine_yxco(cardinal, yxo):
    """psfutil.py:750-753: [2, nsamp, nsamp]."""
    return np.tensordot(cardinal[0] - cardinal[2], yxo[1], axes=0) + np.tensordot(cardinal[1] - cardinal[3], yxo[0], axes=0)


def amp_weight(nfft, a0, a1_samples):
    """The Fourier-mode reweighting of PSFGrp.__init__ (psfutil.py:661-671) on the half spectrum [nfft, nfft/2 + 1];
    a1_samples = cfg.amp_penalty[1] * oversamp."""
    u = np.linspace(0, 1 - 1 / nfft, nfft)
    u = np.where(u > 0.5, u - 1, u)
    u2 = np.square(u)
    ut2 = np.tile(u2[None, : nfft // 2 + 1], (nfft, 1)) + np.tile(u2[:, None], (1, nfft // 2 + 1))
    return 1.0 + a0 * np.exp(-2.0 * np.pi**2 * ut2 * a1_samples**2)


def table_set(psf_in, psf_out, sg, amp=None):
    """Tables of one PSF group in the device's stack order (stamps.PSFGroupTables): the self tables in triangle order, then the
    input-output tables target-major; and C per target.  ``amp`` = (a0, a1 in samples) or None."""
    r_in, r_out = orc.pad_and_rfft2(psf_in, sg.psf), orc.pad_and_rfft2(psf_out, sg.psf)
    if amp is not None:
        w = amp_weight(sg.psf.nfft, amp[0], amp[1])
        r_in, r_out = r_in * w, r_out * w
    io = orc.overlap_cross(r_in, r_out, sg.tab)
    return np.concatenate([orc.overlap_self(r_in, sg.tab), np.moveaxis(io, 1, 0).reshape((-1,) + io.shape[2:])]), orc.overlap_out_C(r_out, sg.tab)


def chain_inputs(g):
    """tests.test_oracle._chain_inputs under psfsplit: the block of tests/golden/stamp_chain*.npz with the sampling positions of
    psfutil.py:739-753 (the block's pixel maps are affine: the four-point positions equal the exact ones to rounding)."""
    n1P, n2, fade, n_inimage, n_inframe = (int(v) for v in g["pars"])
    sg = SplitGeom(int(g["npixpsf"]), int(g["oversamp"]), float(g["dtheta_as"]) / 3600.0, float(g["flat_penalty"]))
    ns, nst = sg.psf.nsamp, n1P + 2
    inst = {(j, i): (g[f"in{j}{i}_x"], g[f"in{j}{i}_y"], g[f"in{j}{i}_data"], g[f"in{j}{i}_cum"].astype(np.int64)) for j in range(nst) for i in range(nst)}
    group_psfs, group_expo = {}, {}
    for gj in range(nst // 2):
        for gi in range(nst // 2):
            used = np.zeros(n_inimage, bool)
            for dj in range(2):
                for di in range(2):
                    used |= np.diff(inst[(2 * gj + dj, 2 * gi + di)][3]) > 0  # psfutil.py:812-818
            p0 = [2 * gi * n2 - 0.5, 2 * gj * n2 - 0.5]  # coadd.py:712
            arr = []
            for e in np.flatnonzero(used):
                M, t0 = g[f"inM{e}"], g[f"int0{e}"]
                card = cardinal_points(lambda xy: np.asarray(xy) @ M.T + t0, p0, sg.psf.oversamp, sg.psf.dscale)
                arr.append(orc.sample_psf(g[f"inpsf{e}"], ns, affine_yxco(card, sg.psf.yxo)))
            group_psfs[(gj, gi)] = orc.finish_psf_group(np.stack(arr), True, True)
            group_expo[(gj, gi)] = [int(e) for e in np.flatnonzero(used)]
    return sg, inst, group_psfs, group_expo, (n1P, n2, fade, n_inimage, n_inframe)


def block_loop(g, kernel, kC, flat_penalty, stamp_neighbours):
    """The reference's stamp loop (coadd.py:2003-2084, 2163-2181) over the whole block of tests/golden/stamp_chain*.npz with PSFSPLIT's
    tables and positions: per stamp _process_input_stamps -> system matrices from the (wide) PSFOvl of its groups -> LA kernel -> map
    tapers -> _perform_coaddition -> accumulation; then the boundary recovery.  ``stamp_neighbours``: blockrun.stamp_neighbours (the
    nine InStamps and pivots of an output stamp).  Returns the block arrays as the reference names them."""
    sg, inst, group_psfs, group_expo, (n1P, n2, fade, n_inimage, n_inframe) = chain_inputs(g)
    sg.set_flat_penalty(flat_penalty)
    ns, nst, n2f = sg.psf.nsamp, n1P + 2, n2 + 2 * fade
    tgt = orc.sample_psf(orc.get_outpsf("GAUSSIAN", 1.1, 2, ns, sg.psf.oversamp), ns, None)[None]
    rft_out = orc.pad_and_rfft2(orc.finish_psf_group(tgt, True, True), sg.psf)
    C = float(orc.overlap_out_C(rft_out, sg.tab)[0])
    rft_in = {k: orc.pad_and_rfft2(v, sg.psf) for k, v in group_psfs.items()}
    rho = float(g["instamp_pad_as"]) / float(g["dtheta_as"])
    kC = np.asarray(kC, dtype=np.float64)
    nside = n1P * n2 + 2 * fade
    out = {k: np.zeros((1, nside, nside), np.float32) for k in ("UC", "Sigma", "kappa", "Tsum", "Neff")}
    out_map = np.zeros((1, n_inframe, nside, nside), np.float32)
    Tw = np.zeros((1, n_inimage, n1P, n1P), np.float32)
    g1 = np.arange(n2f, dtype=np.float64)
    for j in range(1, n1P + 1):
        for i in range(1, n1P + 1):
            ids, pvx, pvy = stamp_neighbours(j, i, n2, nst)
            piv = [(None if np.isnan(a) else a, None if np.isnan(b) else b) for a, b in zip(pvx, pvy)]
            nine = [inst[divmod(int(k), nst)] if k >= 0 else None for k in ids]
            sels = [None if t is None else orc.select_pixels(t[0], t[1], pv, rho) for t, pv in zip(nine, piv)]
            groups = [None if k < 0 else (int(k) // nst >> 1, int(k) % nst >> 1) for k in ids]
            x, y, indata, expo, cum = orc.process_input_stamps(nine, piv, rho)
            ox, oy = (i - 1) * n2 - fade + g1, (j - 1) * n2 - fade + g1
            A, mB = orc.stamp_system_groups(nine, sels, groups, rft_in, rft_out, sg.tab, ox, oy, group_expo)
            if kernel == "Cholesky":
                T, UC, Sg, kp, _ = orc.chol_kernel(A, mB, C, kC, 1e-6, 0.5)
            elif kernel == "Eigen":
                T, UC, Sg, kp, _ = orc.eigen_kernel(A, mB, C, kC, 1e-6, 0.5)
            else:
                raise ValueError(kernel)
            s2 = (n2f, n2f)
            UC, Sg, kp = (np.array(v, dtype=np.float32).reshape(s2).copy() for v in (UC, Sg, kp))
            for a in (kp, Sg, UC):  # coadd.py:1118-1122
                orc.trapezoid(a, fade)
            outimage, Tst, Tin, Neff = orc.perform_coaddition(T[None].copy(), indata, expo, n_inimage, n2f, n2, fade, cum)
            orc.block_accumulate(out_map, outimage, j, i, n2, fade)
            for name, v in (("UC", UC), ("Sigma", Sg), ("kappa", kp), ("Tsum", Tin[0]), ("Neff", Neff[0])):
                orc.block_accumulate(out[name], np.asarray(v, dtype=np.float32)[None], j, i, n2, fade)
            Tw[0, :, j - 1, i - 1] = Tst[0]
    orc.trapezoid_recover(out_map, fade)
    for v in out.values():
        orc.trapezoid_recover(v, fade)
    return {"out_map": out_map, "UC_map": out["UC"], "Sigma_map": out["Sigma"], "kappa_map": out["kappa"], "Tsum_map": out["Tsum"],
            "Neff_map": out["Neff"], "T_weightmap": Tw}
