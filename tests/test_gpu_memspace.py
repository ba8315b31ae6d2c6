"""The memspace contract of the staged C-ABI entries: the same inputs give bit-identical outputs whether the caller passes host
buffers (numpy, IMCOM_MEM_HOST: the library stages them through its workspace) or device buffers (torch tensors on the GPU,
IMCOM_MEM_DEVICE: used in place).  Outputs start from the same non-zero fill in both modes, so elements an entry leaves alone
must keep it in both."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 3.25  # initial value of every floating-point output


class In:  # an input the entry stages (memspace)
    def __init__(self, a):
        self.a = np.ascontiguousarray(a)


class Out(In):  # an output the entry stages (memspace); it starts from FILL
    pass


class HostIn(In):  # a host array in either memory space (per-stamp sizes, C, kappaC, ...)
    pass


class HostOut(In):  # a host output in either memory space (info)
    pass


def _fill(shape, dtype=np.float64):
    return np.full(shape, FILL if np.issubdtype(np.dtype(dtype), np.floating) else 7, dtype=dtype)


def _both(name, args):
    """Call `name` once with host buffers and once with device tensors; return the outputs of the two calls as numpy arrays."""
    import torch

    from pyimcom_amd._lib import MEM_DEVICE, MEM_HOST, check, default_context, lib

    def ptr(b):
        return C.c_void_p(b.data_ptr()) if torch.is_tensor(b) else b.ctypes.data_as(C.c_void_p)

    dev = torch.device("cuda:0")
    ctx = default_context()
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {}
    for mem in (MEM_HOST, MEM_DEVICE):
        bufs, outs, cargs = [], [], []  # (bufs: a device tensor must outlive the call; a bare data_ptr() holds no reference to it)
        for a in args:
            if isinstance(a, In):
                b = a.a.copy()
                if mem == MEM_DEVICE and not isinstance(a, (HostIn, HostOut)):
                    b = torch.from_numpy(b).to(dev)
                bufs.append(b)
                if isinstance(a, (Out, HostOut)):
                    outs.append(b)
                cargs.append(ptr(b))
            else:
                cargs.append(a)
        check(getattr(lib, name)(ctx.handle, *cargs, mem))
        torch.cuda.synchronize(dev)
        res[mem] = [b.cpu().numpy() if torch.is_tensor(b) else b for b in outs]
    return res[MEM_HOST], res[MEM_DEVICE]


def _check_identical(name, args, defined=None):
    """defined: {output index: mask of the elements the entry writes}, for outputs it writes only in part -- what the entry leaves
    alone is the caller's fill in device memory but whatever the workspace held in host memory."""
    host, device = _both(name, args)
    assert len(host) == len(device) > 0
    changed = False
    for q, (h, d) in enumerate(zip(host, device)):
        assert h.dtype == d.dtype and h.shape == d.shape
        if defined and q in defined:
            h, d = h[defined[q]], d[defined[q]]
        assert h.tobytes() == d.tobytes(), f"{name}: output {q} differs between host and device memory ({np.count_nonzero(h != d)} elements)"
        changed |= h.tobytes() != _fill(h.shape, h.dtype).tobytes()
    assert changed, f"{name}: no output was written"
    return host


def _system(rng, ns, m1, ldn):
    """Gaussian overlaps of scattered input pixels and a grid of output pixels (test_gpu_iter_empir._random_case), batched."""
    batch, m = len(ns), m1 * m1
    A, B = np.zeros((batch, ldn, ldn)), np.zeros((batch, m, ldn))
    yx, iy, ix = np.zeros((batch, 2, m)), np.zeros((batch, ldn)), np.zeros((batch, ldn))
    g = np.linspace(2.0, 8.0, m1)
    oy, ox = np.repeat(g, m1), np.tile(g, m1)
    for s, n in enumerate(ns):
        y, x = rng.uniform(0, 10, n), rng.uniform(0, 10, n)
        A[s, :n, :n] = 0.7 * np.exp(-((x[:, None] - x[None]) ** 2 + (y[:, None] - y[None]) ** 2) / 2.0**2)
        B[s, :, :n] = 0.7 * np.exp(-((x[None] - ox[:, None]) ** 2 + (y[None] - oy[:, None]) ** 2) / 2.0**2)
        yx[s] = oy, ox
        iy[s, :n], ix[s, :n] = y, x
    return A, B, yx, iy, ix


NS, M1, LDN = [150, 0, 97], 6, 160
CS = np.array([0.7, 0.65, 0.72])


def _solver_outputs(m):
    batch = len(NS)
    return [Out(_fill((batch, m, LDN), np.float32))] + [Out(_fill((batch, m), np.float32)) for _ in range(3)]


def test_d5512_getw():
    fh = np.random.default_rng(1).uniform(0.0, 1.0, 37)
    _check_identical("imcom_d5512_getw", [In(fh), 37, Out(_fill((37, 10)))])


def test_interp_d5512_keeps_untouched_outputs():
    rng = np.random.default_rng(2)
    tab = rng.standard_normal((2, 40, 37))
    nout = 300
    x, y = rng.uniform(-3.0, 40.0, nout), rng.uniform(-3.0, 43.0, nout)  # off-grid points on every side
    (f,) = _check_identical("imcom_interp_d5512", [In(tab), 2, 40, 37, In(x), In(y), nout, Out(_fill((2, nout))), 0])
    assert np.any(f == FILL) and np.any(f != FILL)  # both modes left the same elements alone (compared bitwise above)


def test_grid_d5512():
    rng = np.random.default_rng(3)
    tab = rng.standard_normal((60, 60))
    npi, nxo, nyo = 5, 12, 10
    x0, y0 = rng.uniform(25.0, 45.0, npi), rng.uniform(25.0, 45.0, npi)
    xp = x0[:, None] - 1.5 * np.arange(nxo)[None, :]
    yp = y0[:, None] - 1.5 * np.arange(nyo)[None, :]
    _check_identical("imcom_grid_d5512", [In(tab), 60, 60, In(xp), In(yp), npi, nxo, nyo, Out(_fill((npi, nxo * nyo)))])


def test_lakernel1(golden):
    g = golden("lakernel1_small")
    m, n = g["mPhalf"].shape
    _check_identical("imcom_lakernel1", [In(g["lam"]), In(g["mPhalf"]), m, n, 0.7, 1e-8, 1e-16, 1e16, 53, Out(_fill(m)), Out(_fill(m)),
                                         Out(_fill(m)), Out(_fill((m, n))), 0.5])


def test_build_reduced_T(golden):
    g = golden("build_reduced_T")
    m, nv = g["brt_a_kappa"].size, g["kappa_nodes"].size
    _check_identical("imcom_build_reduced_T", [In(g["Nflat"]), In(g["Dflat"]), In(g["Eflat"]), In(g["kappa_nodes"]), nv, m,
                                               float(g["brt_a_ucmin"]), float(g["brt_a_smax"]), Out(_fill(m)), Out(_fill(m)),
                                               Out(_fill(m)), Out(_fill(m * nv))])


def test_solve_chol():
    A, B, _, _, _ = _system(np.random.default_rng(4), NS, M1, LDN)
    m = M1 * M1
    _check_identical("imcom_solve_chol", [len(NS), HostIn(np.array(NS, np.int32)), LDN, m, In(A), In(B), HostIn(CS), HostIn(np.array([0.2])), 1,
                                          1e-6, 0.5] + _solver_outputs(m) + [HostOut(_fill(len(NS), np.int32))])


def test_eigh():
    rng = np.random.default_rng(5)
    ldn, ns = 40, [40, 29]
    A = np.zeros((2, ldn, ldn))
    for s, n in enumerate(ns):
        G = rng.standard_normal((n, n))
        A[s, :n, :n] = G + G.T
    _check_identical("imcom_eigh", [2, HostIn(np.array(ns, np.int32)), ldn, In(A), Out(_fill((2, ldn))), Out(_fill((2, ldn, ldn)))])


def test_band_reduce():
    rng = np.random.default_rng(6)
    ldn, ns = 128, [128, 100]
    A = np.zeros((2, ldn, ldn))
    for s, n in enumerate(ns):
        G = rng.standard_normal((n, n))
        A[s, :n, :n] = G + G.T
    bw = 4  # BAND_BW (csrc/launchers.h)
    _check_identical("imcom_band_reduce", [2, HostIn(np.array(ns, np.int32)), ldn, In(A), Out(_fill((2, bw + 1, ldn))), Out(_fill((2, ldn, ldn))),
                                           Out(_fill((2, ldn)))])


def test_solve_eigen():
    A, B, _, _, _ = _system(np.random.default_rng(7), NS, M1, LDN)
    m = M1 * M1
    _check_identical("imcom_solve_eigen", [len(NS), HostIn(np.array(NS, np.int32)), LDN, m, In(A), In(B), HostIn(CS), HostIn(np.array([0.2])), 1,
                                           1e-6, 0.5, 53] + _solver_outputs(m) + [HostOut(_fill(len(NS), np.int32))])


def test_solve_empir():
    A, B, yx, iy, ix = _system(np.random.default_rng(8), NS, M1, LDN)
    m = M1 * M1
    _check_identical("imcom_solve_empir", [len(NS), HostIn(np.array(NS, np.int32)), LDN, m, In(A), In(B), HostIn(CS), 0.2, In(yx), In(iy), In(ix),
                                           2.7, 0] + _solver_outputs(m))


@pytest.mark.parametrize("nv", [1, 3])
def test_solve_iter(nv):
    A, B, yx, iy, ix = _system(np.random.default_rng(9), NS, M1, LDN)
    m = M1 * M1
    kC = np.array([0.2]) if nv == 1 else np.array([0.1, 0.2, 0.4])
    # several kappa nodes: T is combined from the nodes' solutions on the stamps' own n columns only (the padding is not written)
    defined = None if nv == 1 else {0: np.broadcast_to(np.arange(LDN)[None, None, :] < np.array(NS)[:, None, None], (len(NS), m, LDN))}
    _check_identical("imcom_solve_iter", [len(NS), HostIn(np.array(NS, np.int32)), LDN, m, In(A), In(B), HostIn(CS), HostIn(kC), nv, 1e-6, 0.5,
                                          In(yx), In(iy), In(ix), 2.7, 1.5e-3, 30, int(nv > 1)] + _solver_outputs(m), defined)


def _psf_images(rng, count, n):
    yy, xx = np.mgrid[0:n, 0:n] - (n - 1) / 2.0
    return np.stack([np.exp(-(xx**2 + yy**2) / (2 * (2.0 + s) ** 2)) * (1 + 0.01 * rng.standard_normal((n, n))) for s in range(count)])


@pytest.mark.parametrize("with_yxco", [True, False])
def test_sample_psf(with_yxco):
    rng = np.random.default_rng(10)
    psf, ns = _psf_images(rng, 2, 30), 24
    yxco = In(rng.uniform(1.0, 28.0, (2, 2, ns, ns))) if with_yxco else None
    _check_identical("imcom_sample_psf", [2, In(psf), 30, 30, yxco, ns, 0 if with_yxco else 1, 0 if with_yxco else 1, Out(_fill((2, ns, ns)))])


def test_lattice_positions():
    rng = np.random.default_rng(11)
    count, L, ns = 2, 5, 16
    _check_identical("imcom_lattice_positions", [count, L, HostIn(rng.standard_normal((ns, L))), In(rng.standard_normal((count, 2, L, L))), ns,
                                                 Out(_fill((count, 2, ns, ns)))])


def test_psf_gaussian():
    _check_identical("imcom_psf_gaussian", [33, 2.5, 3.0, Out(_fill((33, 33)))])


def test_psf_simple_airy():
    _check_identical("imcom_psf_simple_airy", [24, 5.0, 0.31, 4.0, 1.2, Out(_fill((24, 24)))])


def test_smooth_and_pad():
    from pyimcom_amd._lib import lib

    rng = np.random.default_rng(12)
    n, ny, nx, tw, gs = 2, 20, 17, 2.0, 1.0
    npad = lib.imcom_smooth_pad_width(tw, gs)
    _check_identical("imcom_smooth_and_pad", [n, In(rng.standard_normal((n, ny, nx))), ny, nx, tw, gs, Out(_fill((n, ny + 2 * npad, nx + 2 * npad)))])


def test_select_pixels():
    rng = np.random.default_rng(13)
    npool, n_inframe, batch, ldn = 500, 2, 3, 600
    inst_off = np.array([0, 100, 250, 400, 500], np.int64)
    args = [batch, In(rng.uniform(0, 10, npool)), In(rng.uniform(0, 10, npool)), In(rng.standard_normal((n_inframe, npool)).astype(np.float32)),
            npool, n_inframe, In(rng.integers(0, 5, npool).astype(np.int32)), In(inst_off), len(inst_off) - 1,
            In(rng.integers(-1, 4, (batch, 9)).astype(np.int32)), In(rng.uniform(0, 10, (batch, 9))), In(rng.uniform(0, 10, (batch, 9))), 3.0, ldn,
            Out(_fill((batch, ldn))), Out(_fill((batch, ldn))), Out(_fill((batch, n_inframe, ldn), np.float32)), Out(_fill((batch, ldn), np.int32)),
            Out(_fill((batch, 10), np.int32))]
    _check_identical("imcom_select_pixels", args)


def _nn(Rs):
    from pyimcom_amd._lib import lib

    NN, ng = C.c_int(0), C.c_int(0)
    assert lib.imcom_ginterp_geometry(Rs, 0, C.byref(NN), C.byref(ng), None, None, None) == 0
    return NN.value


def test_ginterp_matrix():
    rng = np.random.default_rng(14)
    Rs, npts, stest = 6.0, 50, 2
    nu = (npts + stest - 1) // stest
    _check_identical("imcom_ginterp_matrix", [Rs, 4.71, npts, In(rng.uniform(0, 1, npts)), In(rng.uniform(0, 1, npts)), HostIn(np.array([0.3, 0.02, 0.3])),
                                              1e-7, stest, Out(_fill((npts, _nn(Rs)))), Out(_fill(nu)), Out(_fill(nu))])


def test_ginterp_resample():
    rng = np.random.default_rng(15)
    nl, n, no = 2, 40, 8
    img = rng.standard_normal((nl, n, n)).astype(np.float32)
    mask = (rng.uniform(0, 1, (n, n)) < 0.02).astype(np.uint8)
    args = [nl, n, n, In(img), 0, In(mask), no, no, HostIn(np.array([15.3, 14.7])), HostIn(np.array([0.9, 0.1, -0.05, 1.02])), 6.0, 4.71,
            HostIn(np.array([0.3, 0.0, 0.3])), 1e-7, 1, 393216, Out(_fill((nl, no, no), np.float32)), Out(_fill((no, no), np.uint8)), Out(_fill(2))]
    _check_identical("imcom_ginterp_resample", args)
