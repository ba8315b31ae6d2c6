"""Destriping on the device: the cost function of ``pyimcom.imdestripe`` and its gradient (reference src/pyimcom/imdestripe.py,
``cost_function`` 1589-1670 and ``residual_function`` 1231-1327) over a mosaic whose SCAs all stay in device memory.

    eng = DestripeEngine(nside, ds_rows, amp_cols=cfg.amp_cols, col_boundary_const=cfg.col_boundary_const)
    for sca in all_scas:
        eng.add_sca(image, mask, g_eff)                  # what Sca_img holds after its masks: float32, bool, float32
    for a, nb in neighbors.items():
        for b in nb:
            eng.set_pair(a, b, x=x_target, y=y_target)   # compareutils.map_sca2sca(wcs_a, wcs_b): positions of a's pixels in b
    eng.bind(imdestripe)                                 # imdestripe.cost_function / residual_function now run here
    imdestripe.conjugate_gradient(...)                   # unchanged

or, from the WCSs alone (seam 21: the gain, the neighbour table and every pair's positions are made on the device, and a pair keeps nothing
of the grid's size):

    for sca in all_scas:
        eng.add_sca(image, mask, wcs=sca.w)              # g_eff = effective_gain(sca.w), made into the engine's own plane
    ov_mat, neighbors = eng.set_pairs_from_wcs(overlap_thresh=0.1, subsamp=8)   # get_overlap_matrix + get_neighbors + set_pair

The host keeps the files, the masks' construction and the optimiser.  csrc/destripe.hip has the kernels;
INTEGRATION.md, seam 8, the binding lines and the quirks that are kept."""

import ctypes as C

import numpy as np

from ._dev import bound_context, is_torch, np_dtype, staged
from ._lib import MEM_DEVICE, ImcomError, check, lib, ptr

__all__ = ["DestripeEngine", "MODELS", "lattice_nodes", "interpolate_bilinear", "transpose_bilinear", "memory_plan", "effective_gain", "formed_pair_bytes"]

IMCOM_ERR_NOMEM = -3
IMCOM_ERR_UNSUPPORTED = -4
MODELS = {"quadratic": 0, "absolute": 1, "huber_loss": 2}
PRIMES = {"quad_prime": "quadratic", "abs_prime": "absolute", "huber_prime": "huber_loss"}
FILL = 0.9  # share of the free device memory a mosaic may take
MAX_L = 33


def _unsupported(msg):
    return ImcomError(IMCOM_ERR_UNSUPPORTED, msg)


def lattice_nodes(nside, L=17):
    """(nodes [L], W [nside, L]): the Chebyshev-Lobatto nodes over the pixel range 0 .. nside - 1 at which a caller evaluates
    ``map_sca2sca`` for ``set_pair(lattice=)`` (row node i, column node j -> pixel (x, y) = (nodes[j], nodes[i])), and the Lagrange weights
    of every pixel index."""
    from .psfs import lattice_nodes_and_weights

    if not 2 <= int(L) <= MAX_L:
        raise _unsupported(f"destripe: a lattice of {L} nodes per axis (2 <= L <= {MAX_L})")
    return lattice_nodes_and_weights(np.arange(int(nside), dtype=np.float64), int(L))


def model_name(f):
    """The cost model a function of the reference stands for (``quadratic`` / ``quad_prime`` ...), by ``__name__``; names pass through."""
    name = f if isinstance(f, str) else getattr(f, "__name__", None)
    name = PRIMES.get(name, name)
    if name not in MODELS:
        raise ValueError(f"destripe: cost model {name!r} is none of {sorted(MODELS)} or their derivatives {sorted(PRIMES)}")
    return name


def _wcs_sizes(n_sca, nside):
    sz = np.zeros(4, dtype=np.int64)
    check(lib.imcom_destripe_wcs_sizes(int(n_sca), int(nside), ptr(sz)))
    return sz


def formed_pair_bytes(nside=4088):
    """What a pair registered with ``keep_positions=False`` keeps on the device: its rotation product, whatever the side."""
    return int(_wcs_sizes(0, nside)[0])


def memory_plan(n_sca, nside, ds_rows, amp_cols, n_full, n_lattice, L, max_np, objmask_setup=0, n_wcs=0, wcs_tables=0, gain_setup=False):
    """Exact device bytes of a mosaic: n_sca SCAs, ``n_full`` ordered pairs with position arrays, ``n_lattice`` with lattices, ``n_wcs``
    whose positions the kernels form from the WCSs (``pairs_wcs``; with any, ``wcs`` counts the descriptor table of the n_sca SCAs and
    ``wcs_tables``, the bytes of the registered WCSs' error tables, each once).  Two psi
    stacks are counted: the one ``cost`` makes (in ``per_sca``) and one uploaded by ``residual`` when psi comes from the host; the bound
    ``cost_function`` lets go of its previous psi before it makes the next.  ``objmask_setup``: the temporaries of the object mask of ONE
    SCA (``objmask.setup_bytes``), a peak during set-up that is not there per SCA; 0 when no SCA asks for one.  ``gain_setup``: some SCA's
    gain is made from its WCS, whose two coordinate frames pass through the workspace."""
    sz = np.zeros(8, dtype=np.int64)
    check(lib.imcom_destripe_sizes(int(n_sca), int(nside), int(ds_rows), int(amp_cols or 0), int(L if n_lattice else 0), int(max_np),
                                   int(n_full + n_lattice + n_wcs), ptr(sz)))
    wz = _wcs_sizes(n_sca, nside)
    nbins = int(sz[0])
    plan = {"nbins": nbins, "per_sca": int(sz[2]), "scas": int(sz[2]) * n_sca, "pairs_full": int(sz[3]) * n_full, "pairs_lattice": int(sz[4]) * n_lattice,
            "pairs_wcs": int(wz[0]) * n_wcs, "wcs": (int(wz[1]) if n_wcs else 0) + int(wcs_tables),
            "weights": int(sz[7]) if n_lattice else 0, "params_and_resids": 8 * n_sca * nbins * 4 + 8 * n_sca,
            "workspace": int(max(sz[5], sz[6], wz[3] if gain_setup else 0)),
            "psi_upload": 4 * n_sca * int(nside) ** 2}  # a psi handed to residual() from the host sits beside the one cost() made
    if objmask_setup:
        plan["objmask_setup"] = int(objmask_setup)
    plan["total"] = sum(v for k, v in plan.items() if k not in ("nbins", "per_sca"))
    return plan


class DestripeEngine:
    """The SCAs of one mosaic, their overlaps and the two functions the reference's optimiser calls."""

    def __init__(self, nside, ds_rows, amp_cols=None, col_boundary_const=0, N_eff_min=0.5, context=None, device="cuda:0", ds_model="constant"):
        self.nside, self.ds_rows = int(nside), int(ds_rows)
        self.amp_cols = int(amp_cols) if amp_cols is not None and amp_cols > 0 else 0
        self.col_boundary_const, self.N_eff_min = float(col_boundary_const), float(N_eff_min)
        if ds_model != "constant":
            raise _unsupported(f"destripe: ds_model={ds_model!r}: the reference's forward_par cannot broadcast its 2 * ds_rows parameters "
                               "(imdestripe.py:690-691), there is nothing to be equal to")
        sz = np.zeros(8, dtype=np.int64)
        check(lib.imcom_destripe_sizes(1, self.nside, self.ds_rows, self.amp_cols, 0, 0, 0, ptr(sz)))  # the shape refusals
        if self.amp_cols and self.col_boundary_const > 0 and self.amp_cols < 50:
            raise _unsupported(f"destripe: the boundary penalty reads 50 columns either side of a boundary, amp_cols={self.amp_cols}")
        self.nbins, self.n_col_blocks = int(sz[0]), int(sz[1])
        self._ctx, self._device = context, device
        self._scas, self._pairs, self.L = [], {}, 0
        self._wcs = []  # per SCA: the DeviceWCS given to add_sca(wcs=) or first named by a formed pair, or None
        self._frozen = self._tables = None
        self._last = None  # (host psi, device psi) of the last cost_function call

    # ---- registration (host logic only) ----
    @property
    def n_sca(self):
        return len(self._scas)

    def add_sca(self, image, mask, g_eff=None, object_mask=None, wcs=None):
        """``object_mask=(threshold_m, threshold_c, type)``: what ``Sca_img.__init__`` does after its masks (imdestripe.py:324-332) happens
        on the device when the mosaic is uploaded -- ``apply_object_mask`` of the image in its own type (float32 or float64), its
        complement and-ed into ``mask``.  The image itself is not zeroed: the reference discards ``image_out`` there.

        ``wcs``: the SCA's WCS (anything ``pyimcom_amd.wcs.as_device_wcs`` takes), the one ``set_pairs_from_wcs`` and formed pairs refer
        to.  With ``g_eff=None`` the gain is ``effective_gain(wcs)``, made at upload into the engine's own plane (no host array)."""
        if self._frozen is not None:
            raise RuntimeError("destripe: the mosaic is already on the device")
        if wcs is not None:
            from .wcs import as_device_wcs

            wcs = as_device_wcs(wcs)
            if wcs.array_shape[-1] != self.nside:
                raise ValueError(f"destripe: the WCS describes an SCA of {wcs.array_shape[-1]} pixels a side, the engine's has {self.nside}")
        if g_eff is None and wcs is None:
            raise ValueError("destripe: an SCA has g_eff=, or wcs= to make it from")
        for arr in (image, mask) + ((g_eff,) if g_eff is not None else ()):
            if tuple(arr.shape) != (self.nside, self.nside):
                raise ValueError(f"destripe: an array of shape {tuple(arr.shape)}, the SCA is {self.nside} x {self.nside}")
        if object_mask is not None:
            threshold_m, threshold_c, kind = object_mask
            if "float32" not in str(image.dtype) and "float64" not in str(image.dtype):
                raise TypeError(f"destripe: the object mask is made of a float32 or float64 image, not {image.dtype}")
            object_mask = (threshold_m, threshold_c, str(kind))
        self._scas.append((image, mask, g_eff, object_mask))
        self._wcs.append(wcs)
        return len(self._scas) - 1

    def set_pair(self, a, b, x=None, y=None, lattice=None, L=None, wcs=None, keep_positions=True):
        """The positions of SCA a's pixels in SCA b: ``x=`` and ``y=`` (the arrays of ``map_sca2sca``), ``lattice=``, or
        ``wcs=(target, ref)`` -- the two WCSs of ``map_sca2sca(all_wcs[a], all_wcs[b])``, anything ``pyimcom_amd.wcs.as_device_wcs`` takes: the
        two float64 arrays are then formed on the device (pyimcom_amd.wcs.map_sca2sca) and kept as the full storage.  Exactly one way.

        ``keep_positions=False`` (with ``wcs=`` only): nothing of the grid's size is kept; the kernels form every position from the two
        descriptors where they use it, the same bits as the stored arrays.  The descriptors are the SCAs': an SCA has one WCS in all its
        formed pairs (and in ``add_sca(wcs=)``)."""
        a, b = int(a), int(b)
        if a == b or min(a, b) < 0 or max(a, b) >= self.n_sca:
            raise ValueError(f"destripe: pair ({a}, {b}) of {self.n_sca} SCAs")
        if (x is None) != (y is None) or (x is not None) + (lattice is not None) + (wcs is not None) != 1:
            raise ValueError("destripe: a pair has x= and y=, or lattice=, or wcs=")
        if not keep_positions and wcs is None:
            raise ValueError("destripe: keep_positions=False goes with wcs=: stored arrays and lattices are what is kept")
        if wcs is not None:
            from .wcs import as_device_wcs

            target, ref = (as_device_wcs(w) for w in wcs)
            if target.array_shape[-1] != self.nside:
                raise ValueError(f"destripe: the target WCS describes an SCA of {target.array_shape[-1]} pixels a side, the engine's has {self.nside}")
            if keep_positions:
                self._pairs[(a, b)] = ("wcs", target, ref)
            else:
                for s, w in ((a, target), (b, ref)):
                    have = self._wcs[s]
                    if have is not None and have is not w and not (np.array_equal(have.descriptor, w.descriptor) and have.table is w.table):
                        raise ValueError(f"destripe: SCA {s} already has another WCS; the formed pairs of an SCA share its one descriptor")
                for s, w in ((a, target), (b, ref)):
                    if self._wcs[s] is None:
                        self._wcs[s] = w
                self._pairs[(a, b)] = ("formed",)
            self._tables = None
            return
        if lattice is not None:
            L = int(L if L is not None else lattice.shape[-1])
            if not 2 <= L <= MAX_L:
                raise _unsupported(f"destripe: a lattice of {L} nodes per axis (2 <= L <= {MAX_L})")
            if tuple(lattice.shape) != (2, L, L) or (self.L and L != self.L):
                raise ValueError(f"destripe: lattice of shape {tuple(lattice.shape)}, expected (2, {self.L or L}, {self.L or L})")
            self.L = L
            self._pairs[(a, b)] = ("lattice", lattice)
        else:
            if int(np.prod(x.shape)) != self.nside ** 2 or int(np.prod(y.shape)) != self.nside ** 2:
                raise ValueError(f"destripe: positions of {int(np.prod(x.shape))} pixels, the SCA has {self.nside ** 2}")
            self._pairs[(a, b)] = ("full", x, y)
        self._tables = None

    @property
    def n_pairs(self):
        return len(self._pairs)

    def neighbors(self):
        nb = {a: [] for a in range(self.n_sca)}
        for a, b in sorted(self._pairs):
            nb[a].append(b)
        return nb

    def set_pairs_from_wcs(self, overlap_thresh=0.1, subsamp=8, pad=0, keep_positions=False):
        """The neighbour table from the WCSs given to ``add_sca(wcs=)``: ``compareutils.get_overlap_matrix`` (pyimcom_amd.wcs), then the
        rule of ``get_neighbors`` (imdestripe.py:1225-1228: ``ov_mat[k, j] >= overlap_thresh and j != k``), and ``set_pair`` for every
        ordered pair found.  Returns ``(ov_mat, neighbors)`` in the reference's types: float32 [n, n] and the dict of lists that
        ``conjugate_gradient(..., neighbors=...)`` takes."""
        from .wcs import get_overlap_matrix

        if self.n_sca == 0 or any(w is None for w in self._wcs):
            raise ValueError("destripe: set_pairs_from_wcs needs every SCA registered with add_sca(wcs=)")
        ov_mat = get_overlap_matrix(self._wcs, pad=pad, subsamp=subsamp, device=self._device, ctx=self._ctx)
        n = self.n_sca
        neighbors = {k: [j for j in range(n) if ov_mat[k, j] >= overlap_thresh and j != k] for k in range(n)}
        for k, nb in neighbors.items():
            for j in nb:
                self.set_pair(k, j, wcs=(self._wcs[k], self._wcs[j]), keep_positions=keep_positions)
        return ov_mat, neighbors

    def _formed_wcs(self):
        """The SCAs that a formed pair names."""
        return sorted({s for k, p in self._pairs.items() if p[0] == "formed" for s in k})

    def plan(self):
        n_lat = sum(1 for p in self._pairs.values() if p[0] == "lattice")
        n_wcs = sum(1 for p in self._pairs.values() if p[0] == "formed")
        nb = self.neighbors()
        tables, seen = 0, set()
        for w in self._wcs:  # each registered WCS's error table once (add_sca(wcs=) and the formed pairs' WCSs: their tables stay on the device)
            t = w.table if w is not None else None
            if t is not None and id(t[0]) not in seen:
                seen.add(id(t[0]))
                tables += 2 * int(t[0].shape[1]) ** 2 * (4 if "float32" in str(t[0].dtype) else 8)
        return memory_plan(max(self.n_sca, 1), self.nside, self.ds_rows, self.amp_cols, len(self._pairs) - n_lat - n_wcs, n_lat, self.L,
                           max([len(v) for v in nb.values()] or [0]), objmask_setup=self._objmask_setup, n_wcs=n_wcs, wcs_tables=tables,
                           gain_setup=any(s is not None and s[2] is None for s in self._scas))

    @property
    def _objmask_setup(self):
        """Bytes of the largest object-mask set-up among the registered SCAs (0: none asks for one; nothing once they are uploaded)."""
        from . import objmask

        return max([objmask.setup_bytes(s[0].shape, np_dtype(s[0]).name, s[3][2]) for s in self._scas if s is not None and s[3] is not None]
                   or [0])

    # ---- device ----
    def _freeze(self):
        import torch

        self.dev = torch.device(self._device)
        ctx = self._ctx = bound_context(self.dev, self._ctx)
        if self._frozen is None:
            if not self._scas:
                raise ValueError("destripe: no SCA registered")
            from .stamps import free_device_bytes

            plan, free = self.plan(), free_device_bytes(self.dev)
            if plan["total"] > FILL * free:
                raise ImcomError(IMCOM_ERR_NOMEM, f"destripe: the mosaic needs {plan['total']} bytes on the device, {free} are free "
                                                   "(streaming SCAs from the host is not served)")
            n, ns = self.n_sca, self.nside
            img = torch.empty((n, ns, ns), dtype=torch.float32, device=self.dev)
            msk = torch.empty((n, ns, ns), dtype=torch.uint8, device=self.dev)
            gef = torch.empty((n, ns, ns), dtype=torch.float32, device=self.dev)
            for i, (im, ma, ge, om) in enumerate(self._scas):
                msk[i].copy_(staged(ma, self.dev, astype=np.bool_))
                if om is None:
                    img[i].copy_(staged(im, self.dev, astype=np.float32))
                else:  # imdestripe.py:324-332: self.mask *= ~object_mask, the image in its own type, image_out discarded
                    from . import objmask

                    own = staged(im, self.dev)
                    omask = objmask.object_mask(own, om[0], om[1], om[2])
                    objmask._apply(ctx, msk[i], omask, msk[i])
                    img[i].copy_(own.to(torch.float32))
                    del own, omask
                if ge is None:  # imdestripe.py:281-297 from the WCS, straight into the plane
                    effective_gain(self._wcs[i], self.nside, device=self.dev, ctx=ctx, out=gef[i])
                else:
                    gef[i].copy_(staged(ge, self.dev, astype=np.float32))
            self._frozen = {"image": img, "mask": msk, "geff": gef, "neff": torch.zeros((n, ns, ns), dtype=torch.float64, device=self.dev),
                            "gmax": float(gef.abs().max().item())}  # set-up, once: the bound the fixed-point scale of the gradient needs
            self._scas = [None] * n
        if self._tables is None:
            from .stamps import free_device_bytes

            new = sum(16 * self.nside ** 2 if p[0] == "wcs" else sum(v.nbytes if not is_torch(v) else 0 for v in p[1:])
                      for p in self._pairs.values())  # pairs not yet on the device (a formed pair brings nothing of that size)
            if new > FILL * free_device_bytes(self.dev):
                raise ImcomError(IMCOM_ERR_NOMEM, f"destripe: the pairs registered since the last evaluation need {new} more bytes on the device")
            keys = sorted(self._pairs)  # the order of the sums: (a, b) ascending, whatever the order of registration
            keep, px, py, pl = [], [], [], []
            rot = np.zeros((max(len(keys), 1), 9), dtype=np.float64)  # R_b R_a^T of the formed pairs, in the table's order
            for i, k in enumerate(keys):
                p = self._pairs[k]
                if p[0] == "formed":
                    check(lib.imcom_destripe_pair_rotation(ptr(self._wcs[k[0]].descriptor), ptr(self._wcs[k[1]].descriptor), ptr(rot[i])))
                    px.append(0), py.append(0), pl.append(0)
                    continue
                if p[0] == "wcs":  # the positions of the whole target grid, formed where they are used
                    from .wcs import map_sca2sca

                    xw, yw, _ = map_sca2sca(p[1], p[2], pad=0, device_out=True, device=self.dev, ctx=ctx)
                    p = ("full", xw.reshape(-1), yw.reshape(-1))
                if p[0] == "full":
                    xs = [staged(v, self.dev, astype=np.float64) for v in p[1:]]
                    self._pairs[k] = ("full", xs[0], xs[1])
                    keep += xs
                    px.append(xs[0].data_ptr()), py.append(xs[1].data_ptr()), pl.append(0)
                else:
                    la = staged(p[1], self.dev, astype=np.float64)
                    self._pairs[k] = ("lattice", la)
                    keep.append(la)
                    px.append(0), py.append(0), pl.append(la.data_ptr())
            W = torch.as_tensor(lattice_nodes(self.nside, self.L)[1], device=self.dev) if self.L else None
            arr = lambda v: np.asarray(v, dtype=np.uint64)  # noqa: E731
            wcs = [None] * 7  # the WCS arguments of the three entries (include/imcom_hip.h): none when no pair is formed
            formed = self._formed_wcs()
            if formed:
                from .wcs import DESC_LEN

                desc = np.zeros((self.n_sca, DESC_LEN), dtype=np.float64)
                tab = [(0, 0, 0, 0.0, 0.0)] * self.n_sca
                for s in formed:
                    desc[s] = self._wcs[s].descriptor
                    ta = self._wcs[s]._table_args(self.dev)  # (the DeviceWCS keeps its table's tensor: one a WCS, whatever its pairs)
                    tab[s] = (ta[0].value if ta[0] is not None else 0,) + tuple(ta[1:])
                desc_d, rot_d = torch.as_tensor(desc).to(self.dev), torch.as_tensor(rot).to(self.dev)
                keep += [desc_d, rot_d]
                wcs = [desc_d]
                if any(t[0] for t in tab):
                    wcs += [arr([t[0] for t in tab]), np.asarray([t[1] for t in tab], dtype=np.int32), np.asarray([t[2] for t in tab], dtype=np.int32),
                            np.asarray([t[3] for t in tab], dtype=np.float64), np.asarray([t[4] for t in tab], dtype=np.float64)]
                else:
                    wcs += [None] * 5
                wcs.append(rot_d)
            self._tables = {"n": len(keys), "a": np.asarray([k[0] for k in keys], dtype=np.int32), "b": np.asarray([k[1] for k in keys], dtype=np.int32),
                            "x": arr(px), "y": arr(py), "lat": arr(pl), "W": W, "keep": keep, "wcs": [ptr(v) for v in wcs], "wcs_keep": wcs}
            t, f = self._tables, self._frozen
            check(lib.imcom_destripe_neff(ctx.handle, self.n_sca, self.nside, self.L, ptr(f["mask"]), t["n"], ptr(t["a"]), ptr(t["b"]), ptr(t["x"]),
                                          ptr(t["y"]), ptr(t["lat"]), ptr(W), ptr(f["neff"]), *t["wcs"]))
        return self._frozen, self._tables

    @property
    def N_eff(self):
        return self._freeze()[0]["neff"]

    def _model(self, model, thresh):
        name = model_name(model)
        if name == "huber_loss" and thresh is None:
            raise ValueError("destripe: huber_loss needs a threshold")
        return MODELS[name], float(thresh) if thresh is not None else 0.0

    def cost(self, params, model="quadratic", thresh=None):
        """(epsilon, psi): psi a device tensor [n_sca, nside, nside] float32; epsilon the sum of the SCAs' costs in index order."""
        import torch

        m, th = self._model(model, thresh)
        f, t = self._freeze()
        params = staged(params, self.dev, astype=np.float64)
        if tuple(params.shape) != (self.n_sca, self.nbins):
            raise ValueError(f"destripe: params of shape {tuple(params.shape)}, expected {(self.n_sca, self.nbins)}")
        psi = torch.empty((self.n_sca, self.nside, self.nside), dtype=torch.float32, device=self.dev)
        eps = torch.empty(self.n_sca, dtype=torch.float64, device=self.dev)
        check(lib.imcom_destripe_cost(self._ctx.handle, self.n_sca, self.nside, self.ds_rows, self.amp_cols, self.L, ptr(f["image"]), ptr(f["mask"]),
                                      ptr(f["geff"]), ptr(f["neff"]), ptr(params), t["n"], ptr(t["a"]), ptr(t["b"]), ptr(t["x"]), ptr(t["y"]), ptr(t["lat"]),
                                      ptr(t["W"]), m, th, self.N_eff_min, self.col_boundary_const, ptr(psi), ptr(eps), *t["wcs"]))
        epsilon = 0.0
        for e in eps.cpu().numpy():  # (the copy waits for the stream: `params` may go)
            epsilon += float(e)
        return epsilon, psi

    def residual(self, psi, model="quadratic", thresh=None, extrareturn=False):
        """resids [n_sca, nbins] float64 (numpy) for the psi of ``cost``; with ``extrareturn`` also -term_1 and term_2 on their own."""
        import torch

        m, th = self._model(model, thresh)
        f, t = self._freeze()
        psi = staged(psi, self.dev, astype=np.float32)
        if tuple(psi.shape) != (self.n_sca, self.nside, self.nside):
            raise ValueError(f"destripe: psi of shape {tuple(psi.shape)}")
        out = torch.empty((3 if extrareturn else 1, self.n_sca, self.nbins), dtype=torch.float64, device=self.dev)
        check(lib.imcom_destripe_residual(self._ctx.handle, self.n_sca, self.nside, self.ds_rows, self.amp_cols, self.L, ptr(psi), ptr(f["geff"]),
                                          ptr(f["neff"]), t["n"], ptr(t["a"]), ptr(t["b"]), ptr(t["x"]), ptr(t["y"]), ptr(t["lat"]), ptr(t["W"]), m, th,
                                          f["gmax"], ptr(out[0]), ptr(out[1]) if extrareturn else None, ptr(out[2]) if extrareturn else None, *t["wcs"]))
        res = out.cpu().numpy()
        return (res[0], res[1], res[2]) if extrareturn else res[0]

    # ---- the reference's two functions (signatures and return types of imdestripe.py:1589-1591, 1231-1243) ----
    def _check_mosaic(self, scalist, neighbors):
        if len(scalist) != self.n_sca:
            raise ValueError(f"destripe: {len(scalist)} SCAs in scalist, {self.n_sca} on the device")
        mine = self.neighbors()
        if {k: sorted(v) for k, v in neighbors.items() if v} != {k: v for k, v in mine.items() if v}:
            raise ValueError("destripe: `neighbors` is not the set of pairs registered with set_pair")

    def cost_function(self, p, f, thresh, workers, scalist, neighbors, cfg, tempdir=None, of=None, indata_type="fits"):
        self._check_mosaic(scalist, neighbors)
        self._last = None  # the previous psi goes back to the allocator before the next one is made
        epsilon, psi = self.cost(np.reshape(p.params, (self.n_sca, self.nbins)), model_name(f), thresh)
        host = psi.cpu().numpy()
        self._last = (host, psi)
        return epsilon, host

    def residual_function(self, psi, f_prime, scalist, wcslist, neighbors, thresh, workers, cfg, extrareturn=False, of=None, indata_type="fits"):
        self._check_mosaic(scalist, neighbors)
        if self._last is not None and psi is self._last[0]:
            psi = self._last[1]  # the array cost_function handed out: its device copy is still here
        return self.residual(psi, model_name(f_prime), thresh, extrareturn=extrareturn)

    def bind(self, module):
        """Replace ``module.cost_function`` and ``module.residual_function`` (pyimcom.imdestripe) by this engine's."""
        module.cost_function = self.cost_function
        module.residual_function = self.residual_function
        return module


def effective_gain(wcs, nside=4088, dtype=np.float32, device_out=False, device="cuda:0", ctx=None, out=None):
    """``Sca_img``'s effective gain from its WCS (imdestripe.py:281-297 with ``get_coordinates(pad=2.0)``, 451-474) on the device: (ra, dec)
    in degrees of the ``(nside + 2)^2`` frame, the four centred differences, their determinant, ``1 / (|det| cos(dec))``.  ``wcs``: anything
    ``pyimcom_amd.wcs.as_device_wcs`` takes.  dtype float32 (the reference's ``use_output_float``) or float64.  Kept from 292-293: the
    determinants come back transposed against ``dec`` (seam 8).  ``out``: a contiguous device tensor [nside, nside] of
    that dtype to write into."""
    import torch

    from .wcs import as_device_wcs

    w, nside = as_device_wcs(wcs), int(nside)
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"destripe: a gain as {dtype}; served are float32 and float64")
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    dev = torch.device(device if out is None else out.device)
    ctx = bound_context(dev, ctx)
    if out is None:
        out = torch.empty((nside, nside), dtype=tdt, device=dev)
    elif tuple(out.shape) != (nside, nside) or out.dtype != tdt or not out.is_contiguous():
        raise ValueError(f"destripe: out of shape {tuple(out.shape)} and type {out.dtype}, expected a contiguous ({nside}, {nside}) of {tdt}")
    tab = w._table_args(dev)
    check(lib.imcom_wcs_effective_gain(ctx.handle, ptr(w.descriptor), tab[0], tab[1], tab[2], tab[3], tab[4], nside, ptr(out), int(dtype == np.float32), MEM_DEVICE))
    return out if device_out else out.cpu().numpy()


def _f64(a, dev):
    return staged(a, dev, astype=np.float64)


def interpolate_bilinear(image, g_eff, x, y, out=None, device="cuda:0", ctx=None):
    """``bilinear_interpolation(image, g_eff, coords, out)`` as imdestripe.py:972-998 calls it, coords = (y, x) columns: out (flat order of
    x, y) += the bilinear value of image * g_eff.  float64 in and out; returns a device tensor of x's shape."""
    import torch

    dev = torch.device(device)
    ctx = bound_context(dev, ctx)
    src, gs, xs, ys = (_f64(v, dev) for v in (image, g_eff, x, y))
    res = torch.zeros(xs.shape, dtype=torch.float64, device=dev) if out is None else _f64(out, dev).clone()
    check(lib.imcom_destripe_interp(ctx.handle, ptr(src), ptr(gs), int(src.shape[0]), int(src.shape[1]), ptr(xs), ptr(ys), C.c_long(xs.numel()), ptr(res)))
    torch.cuda.current_stream(dev).synchronize()
    return res


def transpose_bilinear(image, x, y, shape, device="cuda:0", ctx=None):
    """``bilinear_transpose(image, coords, original_image)`` (imdestripe.py:1001-1023) into a zero image of ``shape``."""
    import torch

    dev = torch.device(device)
    ctx = bound_context(dev, ctx)
    img, xs, ys = (_f64(v, dev) for v in (image, x, y))
    res = torch.zeros(tuple(shape), dtype=torch.float64, device=dev)
    check(lib.imcom_destripe_interp_transpose(ctx.handle, ptr(img), ptr(xs), ptr(ys), C.c_long(img.numel()), int(shape[0]), int(shape[1]), ptr(res)))
    torch.cuda.current_stream(dev).synchronize()
    return res
