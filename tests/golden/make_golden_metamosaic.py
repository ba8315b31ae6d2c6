"""Writes tests/golden/metamosaic.npz (seam 19).  The reference's own class ``MetaMosaic`` (src/pyimcom/meta/distortimage.py) is taken out
of the syntax tree -- the module imports astropy at top level -- and executed with stand-ins for what it imports: an in-memory ``ReadFile``
that maps file names to HDU-like objects (``.data``, ``.header["UNIT"]``, ``.header.comments``), tests/wcs_reference.py's numpy chain for the
WCS, a ``ginterp.MultiInterp`` that records its arguments, and the reference's ``helper.HDU_to_bels`` imported by file path.  Recorded: the
four arrays of every mosaic case and the windows the constructor printed; the masks after each mask method; ``origimage``'s and
``shearimage``'s dicts and the arguments handed to the resampler; the masks of the cap cases from the loop of lines 340-352.

A cap case in which a tested pixel has |d^2 - r^2| <= 1e-12 r^2 (np.longdouble) is refused: above that margin every faithful ``hypot`` decides
alike.  A ``mask_caps`` case where a position of the numpy chain lies within 1e-6 pixel of changing a box bound or a pixel's membership is
refused as well.  Run from the repository root with the reference's package directory in PYIMCOM_REFERENCE:
    PYIMCOM_REFERENCE=.../src/pyimcom python tests/golden/make_golden_metamosaic.py"""

import ast
import contextlib
import importlib.util
import io
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import metamosaic_reference as MR  # noqa: E402
from tests import wcs_reference as RW  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metamosaic.npz")
MARGIN, EDGE = 1e-12, 1e-6

CFG = {"n1": 4, "n2": 8, "postage_pad": 1, "nblock": 4, "dtheta": 0.04 / 3600.0, "ra": 53.0, "dec": -40.0, "lonpole": 180.0, "outpsf": "GAUSSIAN",
       "sigmatarget": 1.5 / 2.355, "extrainput": [None, "truth,x", "whitenoise1"]}
BLOCK_SIDE = (CFG["n1"] + 2 * CFG["postage_pad"]) * CFG["n2"]  # 48
STEM = "mem/mosaic_F"
# (name, ix, iy, nlayer, dtype, bbox, extpix, variant)
MOSAICS = [
    ("interior", 1, 2, 3, "float32", None, None, ""),
    ("corner", 0, 3, 1, "float32", None, None, ""),
    ("bbox", 1, 1, 1, "float32", [0, 2, 0, 4], None, ""),
    ("ext10", 2, 1, 3, "float32", None, 10, ""),
    ("ext0", 1, 1, 1, "float32", None, 0, ""),
    ("double", 2, 1, 1, "float64", None, None, ""),
    ("bytes", 1, 2, 1, "float32", None, None, "u8"),
]
# units of (in_x, in_y): (FIDELITY unit, comment, SIGMA unit, comment); everything else has the plain ones
FID_COMMENT, SIG_COMMENT = "leakage U/C", "noise amplification"
UNITS = {(1, 1): ("unknown", FID_COMMENT, MR.SIG_UNIT, SIG_COMMENT), (2, 2): ("0.2mB", "-0.2 mB: legacy sign", MR.SIG_UNIT, SIG_COMMENT),
         (0, 2): (MR.FID_UNIT, FID_COMMENT, "0.5 dB", SIG_COMMENT)}
SHEARS = [  # name, N, jac, psfgrow, oversamp, fidelity_min, select_layers
    ("identity", 24, None, 1.0, 1.0, None, None),
    ("rotation", 25, [[np.cos(np.radians(20.0)), -np.sin(np.radians(20.0))], [np.sin(np.radians(20.0)), np.cos(np.radians(20.0))]], 1.02, 1.0, 30.1, None),
    ("shear", 40, [[1.02, 0.01], [0.01, 0.98]], 1.05, 2.0, None, [2, 0]),
]
ORIGS = [("interior", None, None), ("interior", 33, None), ("interior", 31, [2, 0]), ("interior", 98, None), ("ext10", 20, None), ("ext10", 51, [1])]
CAPS = {  # name: (x, y, r) on a 96 x 96 mask
    "inside": ([40.3], [50.7], [9.2]),
    "left": ([2.2], [40.1], [6.4]),
    "right": ([93.6], [30.3], [5.7]),
    "bottom": ([33.3], [1.4], [4.9]),
    "top": ([60.8], [94.9], [7.3]),
    "corner": ([94.2], [95.1], [8.6]),
    "outside": ([140.2], [-60.4], [12.3]),
    "outside_near": ([-3.6], [50.2], [2.3]),
    "r0": ([10.5], [20.25], [0.0]),
    "between": ([30.5], [40.5], [0.3]),
    "on_centre": ([40.0], [50.0], [0.3]),
    "overlap": ([20.2, 26.9], [70.4, 73.1], [6.1, 5.2]),
    "huge": ([47.3], [48.9], [150.4]),
    "none": ([], [], []),
    "negative_r": ([50.2], [50.3], [-2.4]),
}


def random_caps():
    rng = np.random.default_rng(19)
    return rng.uniform(-10.0, 106.0, 1000), rng.uniform(-10.0, 106.0, 1000), rng.uniform(0.0, 6.0, 1000)


# ---- stand-ins ---------------------------------------------------------------------------------------------------------------------------

class Header(dict):
    def __init__(self, unit, comment):
        super().__init__(UNIT=unit)
        self.comments = {"UNIT": comment}


class HDU:
    def __init__(self, data, header=None):
        self.data, self.header = data, header


FILES = {}


class ReadFile:
    def __init__(self, fname):
        self.fname = fname

    def __enter__(self):
        return FILES[self.fname]

    def __exit__(self, *a):
        return False


class Cfg:
    def __init__(self, text=None):
        for k, v in CFG.items():
            setattr(self, k, v)
        self.Nside = self.n1 * self.n2


class Settings:  # config.py:85-97
    degree = np.pi / 180.0
    arcmin = degree / 60.0
    arcsec = arcmin / 60.0
    pixscale_native = 0.11 * arcsec


class _Inner:
    pass


class NumpyWCS:
    """``astropy.wcs.WCS`` as distortimage.py uses it: attributes of ``.wcs`` or a header dict, evaluated by tests/wcs_reference.py's chain."""

    def __init__(self, header=None, naxis=2):
        self.header = dict(header) if header is not None else None
        self.wcs = _Inner()

    def as_header(self):
        if self.header is not None:
            return self.header
        w = self.wcs
        return {"CTYPE1": w.ctype[0], "CTYPE2": w.ctype[1], "CRPIX1": w.crpix[0], "CRPIX2": w.crpix[1], "CDELT1": w.cdelt[0], "CDELT2": w.cdelt[1],
                "CRVAL1": w.crval[0], "CRVAL2": w.crval[1], "LONPOLE": w.lonpole}

    def desc(self):
        from pyimcom_amd import wcs as W

        return W.DeviceWCS.from_header(self.as_header()).descriptor

    def all_pix2world(self, x, y, origin):
        return RW.np_pix2world(self.desc(), None, np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), origin)

    def all_world2pix(self, pos, origin):
        x, y, ok = RW.np_world2pix(self.desc(), None, pos[:, 0], pos[:, 1], origin)
        assert np.all(ok)
        return np.stack((x, y), axis=1)


class WcsModule:
    WCS = NumpyWCS


class Resampler:
    calls = []

    @classmethod
    def MultiInterp(cls, in_array, in_mask, out_size, out_origin, out_transform, Rsearch, samp, Cov):
        cls.calls.append({"in_array": np.array(in_array), "in_mask": np.array(in_mask), "out_size": list(out_size), "opos": np.array(out_origin, dtype=np.float64),
                          "J": np.array(out_transform, dtype=np.float64), "Rsearch": float(Rsearch), "samp": float(samp), "C": [float(v) for v in Cov]})
        return np.zeros((np.shape(in_array)[0],) + tuple(out_size), dtype=in_array.dtype), np.zeros(tuple(out_size), dtype=bool), 0.0, 0.0


def reference_code():
    ref = os.environ["PYIMCOM_REFERENCE"]
    spec = importlib.util.spec_from_file_location("pyimcom_helper", os.path.join(ref, "diagnostics", "outimage_utils", "helper.py"))
    helper = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(helper)
    tree = ast.parse(open(os.path.join(ref, "meta", "distortimage.py")).read(), filename="distortimage.py")
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MetaMosaic")
    caps = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "mask_caps")
    loop = next(n for n in caps.body if isinstance(n, ast.For) and n.lineno == 340 and n.end_lineno == 352)
    cls.body = [n for n in cls.body if not (isinstance(n, ast.FunctionDef) and n.name == "to_file")]  # (FITS)
    ns = {"np": np, "wcs": WcsModule, "ReadFile": ReadFile, "Config": Cfg, "Settings": Settings, "HDU_to_bels": helper.HDU_to_bels, "ginterp": Resampler}
    exec(compile(ast.Module(body=[cls], type_ignores=[]), "distortimage.py", "exec"), ns)
    return helper, ns["MetaMosaic"], compile(ast.Module(body=[loop], type_ignores=[]), "distortimage.py", "exec")


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

def block_inputs():
    """The sixteen synthetic block files: name_xx_yy -> (primary [3, 48, 48] f32, fidelity u16, sigma i16)."""
    return {(bx, by): MR.synthetic_block(100 + 4 * by + bx, 3, BLOCK_SIDE, BLOCK_SIDE) for bx in range(CFG["nblock"]) for by in range(CFG["nblock"])}


def fill_files(blocks, nlayer, dtype, variant):
    FILES.clear()
    for (bx, by), (p, fid, sig) in blocks.items():
        fu, fc, su, sc = UNITS.get((bx, by), (MR.FID_UNIT, FID_COMMENT, MR.SIG_UNIT, SIG_COMMENT))
        prim = p[:nlayer] if dtype == "float32" else MR.to_float64(p[:nlayer])
        FILES[f"{STEM}_{bx:02d}_{by:02d}.fits"] = {"CONFIG": HDU({"text": ["#"]}), "PRIMARY": HDU(prim[None]),
                                                   "FIDELITY": HDU((MR.to_uint8(fid) if variant == "u8" else fid)[None], Header(fu, fc)), "SIGMA": HDU(sig[None], Header(su, sc))}


plain = MR.plain


def image_dict(prefix, im, out):
    out[prefix + "_image"], out[prefix + "_mask"] = np.array(im["image"]), np.array(im["mask"])
    return {"pars": plain(im["pars"]), "layers": im["layers"], "psf_fwhm": float(im["psf_fwhm"]), "ref": plain(im["ref"]), "header": plain(im["wcs"].header)}


def compute():
    import warnings

    helper, MetaMosaic, cap_loop = reference_code()
    blocks = block_inputs()
    out, meta = {}, {"cfg": CFG, "stem": STEM, "block_side": BLOCK_SIDE, "mosaics": [], "units": {f"{k[0]},{k[1]}": v for k, v in UNITS.items()}, "margin": MARGIN, "edge": EDGE}
    for (bx, by), (p, fid, sig) in blocks.items():
        out[f"block_{bx}_{by}_primary"], out[f"block_{bx}_{by}_fidelity"], out[f"block_{bx}_{by}_sigma"] = p, fid, sig
    fill_files(blocks, 3, "float32", "")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        meta["bels"] = {f"{bx},{by}": [helper.HDU_to_bels(FILES[f"{STEM}_{bx:02d}_{by:02d}.fits"][k]) for k in ("FIDELITY", "SIGMA")] for bx, by in blocks}
    mosaics = {}
    for name, ix, iy, nlayer, dtype, bbox, extpix, variant in MOSAICS:
        fill_files(blocks, nlayer, dtype, variant)
        log = io.StringIO()
        with contextlib.redirect_stdout(log), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (the legacy-sign note of HDU_to_bels)
            m = MetaMosaic(f"{STEM}_{ix:02d}_{iy:02d}.fits", bbox=bbox, extpix=extpix, verbose=True)
        wins = []
        for ln in log.getvalue().splitlines():
            g = re.match(r"IN\s*(-?\d+),\s*(-?\d+) \[\s*(-?\d+):\s*(-?\d+),\s*(-?\d+):\s*(-?\d+)\] offset x=\s*(-?\d+) y=\s*(-?\d+)", ln)
            if g:
                in_x, in_y, symin, symax, sxmin, sxmax, cx, cy = (int(v) for v in g.groups())
                wins.append([in_x - ix, in_y - iy, in_x, in_y, symin, symax, sxmin, sxmax, cx, cy])
        assert m.nlayer == nlayer and str(m.im_dtype) == dtype and m.in_image.dtype == np.dtype(dtype) and m.in_fidelity.dtype == np.float32
        out[name + "_image"], out[name + "_fidelity"], out[name + "_noise"], out[name + "_mask"] = m.in_image, m.in_fidelity, m.in_noise, m.in_mask
        meta["mosaics"].append({"name": name, "ix": ix, "iy": iy, "nlayer": nlayer, "dtype": dtype, "bbox": bbox, "extpix": extpix, "variant": variant,
                                "trunc": int(m.trunc), "Nside": int(m.Nside), "windows": wins, "header": plain(m.wcs.as_header())})
        mosaics[name] = m
        print(f"{name}: Nside {m.Nside}, trunc {m.trunc}, {len(wins)} blocks, {int(m.in_mask.sum())} masked, {int(np.isnan(m.in_fidelity).sum())} NaN fidelities", flush=True)

    # the mask methods, one after the other, on the interior mosaic
    m = mosaics["interior"]
    first = m.in_mask.copy()
    extramask = np.random.default_rng(5).random(first.shape) < 0.05
    m.mask_fidelity_cut(30.1)
    out["cut_fidelity"] = m.in_mask.copy()
    m.mask_noise_cut(2.9)
    out["cut_noise"] = m.in_mask.copy()
    m.maskpix(extramask)
    out["cut_extra"], out["extramask"] = m.in_mask.copy(), extramask
    meta["cuts"] = {"fidelitymin": 30.1, "noisemax": 2.9}
    m.in_mask = first.copy()

    # origimage and shearimage
    meta["orig"] = []
    for k, (on, N, sel) in enumerate(ORIGS):
        entry = {"mosaic": on, "N": N, "select_layers": sel}
        try:
            entry.update(image_dict(f"orig{k}", mosaics[on].origimage(N=N, select_layers=sel), out), raises=False)
        except ValueError as e:
            entry.update(raises=True, message=str(e))
        meta["orig"].append(entry)
    meta["shear"] = []
    for name, N, jac, psfgrow, oversamp, fmin, sel in SHEARS:
        Resampler.calls.clear()
        im = m.shearimage(N, jac=None if jac is None else np.array(jac), psfgrow=psfgrow, oversamp=oversamp, fidelity_min=fmin, select_layers=sel)
        (call,) = Resampler.calls
        ul = list(range(3)) if sel is None else sel
        assert np.array_equal(call["in_array"].view(np.uint32), m.in_image[ul].view(np.uint32))
        out[f"shear_{name}_inmask"], out[f"shear_{name}_opos"], out[f"shear_{name}_J"] = call["in_mask"], call["opos"], call["J"]
        d = image_dict(f"shear_{name}", im, out)
        del out[f"shear_{name}_image"], out[f"shear_{name}_mask"]  # (the recording resampler's zeros)
        for key in ("UMAX", "SMAX"):
            del d["pars"][key]
        meta["shear"].append(dict(d, name=name, N=N, jac=plain(jac), psfgrow=psfgrow, oversamp=oversamp, fidelity_min=fmin, select_layers=sel, ul=ul,
                                  out_size=call["out_size"], Rsearch=call["Rsearch"], samp=call["samp"], C=call["C"]))

    # the circles (340-352), each case on an empty 96 x 96 mask
    class Holder:
        pass

    cases = dict(CAPS, random=random_caps())
    meta["caps"] = []
    for name, (x, y, r) in cases.items():
        x, y, r = (np.asarray(v, dtype=np.float64) for v in (x, y, r))
        margin = MR.cap_margin(x, y, r, 96)
        if margin <= MARGIN:
            raise SystemExit(f"cap case {name}: a tested pixel within {margin:.2e} r^2 of the circle; choose another case")
        h = Holder()
        h.in_mask = np.zeros((96, 96), dtype=bool)
        exec(cap_loop, {"np": np, "self": h, "x_": x, "y_": y, "r_": r, "N": len(x), "ns": 96})
        out[f"caps_{name}_xyr"], out[f"caps_{name}_mask"] = np.stack((x, y, r)), h.in_mask
        meta["caps"].append({"name": name, "n": len(x), "hits": int(h.in_mask.sum()), "margin": margin if np.isfinite(margin) else None})
        print(f"caps {name}: {len(x)} objects, {int(h.in_mask.sum())} pixels, margin {margin:.2e}", flush=True)

    # mask_caps from (ra, dec, radius) on the interior mosaic; an array of radii and one radius for all
    w = m.wcs
    rng = np.random.default_rng(7)
    px = np.concatenate((rng.uniform(-20.0, 116.0, 40), [3000.31, -2500.61, 48.2]))  # (two far outside the preselection of 314-331)
    py = np.concatenate((rng.uniform(-20.0, 116.0, 40), [40.3, 7000.4, 47.7]))
    ra, dec = w.all_pix2world(px, py, 0)
    radius = np.concatenate((rng.uniform(0.5, 9.0, 40), [5.13, 5.21, 30.37])) * CFG["dtheta"]
    meta["sky"] = []
    for name, rad in (("array", radius), ("scalar", 4.37 * CFG["dtheta"])):
        pos = w.all_world2pix(np.vstack((ra, dec)).T, 0)
        rr = (np.zeros_like(ra) + rad) / CFG["dtheta"]
        near = [np.abs(v - np.round(v)).min() for v in (pos[:, 0] - rr, pos[:, 0] + rr, pos[:, 1] - rr, pos[:, 1] + rr)]
        iy_, ix_ = np.mgrid[0:96, 0:96]
        ring = min(float(np.min(np.abs(np.hypot(ix_ - pos[j, 0], iy_ - pos[j, 1]) - rr[j]))) for j in range(len(ra)))
        if min(near) < EDGE or ring < EDGE:
            raise SystemExit(f"mask_caps {name}: a position within {min(min(near), ring):.2e} pixel of a box bound or of a pixel's membership")
        before = m.in_mask.copy()
        m.mask_caps(ra, dec, rad)
        out[f"sky_{name}_mask"] = m.in_mask.copy()
        meta["sky"].append({"name": name, "added": int(m.in_mask.sum() - before.sum()), "edge": float(min(min(near), ring))})
        print(f"mask_caps {name}: {meta['sky'][-1]['added']} pixels added, {meta['sky'][-1]['edge']:.2e} from an edge", flush=True)
        m.in_mask = before
    out["sky_ra"], out["sky_dec"], out["sky_radius"], out["sky_scalar_radius"] = ra, dec, radius, np.float64(4.37 * CFG["dtheta"])
    out["meta"] = np.array(json.dumps(meta))
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **compute())
    print(OUT, os.path.getsize(OUT), "bytes")
