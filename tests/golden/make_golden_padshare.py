"""Writes tests/golden/padshare.npz (seam 20).  The reference's own ``OutImage._update_hdu_data`` and ``OutImage.get_output_map``
(src/pyimcom/analysis.py:394-537, 344-392) and ``Mosaic.share_padding_stamps`` (1429-1467) are taken out of the syntax tree -- the module
imports astropy at top level -- and run with stand-ins: in-memory HDU objects (``.data``, ``.header["UNIT"]``, ``.header.comments["UNIT"]``),
a ``Config`` stand-in, the INDATA columns as a dict, and a ``_load_or_save_hdu_list`` that only records the call.  ``OutStamp.trapezoid`` and
``Block.compress_map`` are the reference's own functions out of coadd.py's tree, ``HDU_to_bels`` the reference's helper imported by path.

Recorded: the inputs; every block of the mosaic case after the full loop and the order of its loads, updates and saves; for every pair case
my strip of every array after each call, flattened and stacked over the eight calls; the float32 sums of every map strip before the encode (the reference's ``compress_map`` is wrapped
to record its argument).  Asserted before anything is written: tests/padshare_reference.py reproduces all of it bit for bit, with
``zero_floor=None`` and with whichever forced setting the installed numpy produces (the other setting is the restatement's alone and is
not recorded).  The codes of an add call may differ from the device's encode (log10 correctly rounded to float32) by one
count where numpy's float32 log10 is not correctly rounded: the share of such pixels per map strip is measured on the fixture's own sums,
stored, and a fixture in which it exceeds 1 % or any code differs by more than one count is refused.  Run from the repository root with the
reference's package directory in PYIMCOM_REFERENCE:
    PYIMCOM_REFERENCE=.../src/pyimcom python tests/golden/make_golden_padshare.py"""

import ast
import contextlib
import importlib.util
import io
import json
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import padshare_reference as PR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "padshare.npz")
CAP = 0.01
MOSAIC = {"n2": 4, "postage_pad": 2, "n1P": 8, "fk": 2, "nblock": 3, "n_out": 2, "nlayer": 3, "outmaps": "USKTN"}
# the exposures of block (iby, ibx): lists that differ in length and order; (1, 0) and (2, 0) share none; (0, 1) repeats (11, 3)
IDSCAS = {(0, 0): [(11, 3), (12, 5), (13, 7)], (0, 1): [(12, 5), (11, 3), (14, 1), (11, 3)], (0, 2): [(14, 1), (15, 2)],
          (1, 0): [(13, 7), (11, 3), (16, 9), (12, 5)], (1, 1): [(16, 9), (12, 5), (11, 3)], (1, 2): [(15, 2), (16, 9), (14, 1)],
          (2, 0): [(21, 4), (22, 6)], (2, 1): [(22, 6), (16, 9), (12, 5), (21, 4), (11, 3)], (2, 2): [(16, 9), (21, 4), (15, 2)]}
# pair cases: name -> (n2, postage_pad, n1P, fk, outmaps, legacy); each runs the eight direction x add_mode combinations
PAIRS = {"fk0": (4, 1, 4, 0, "USKTN", False), "fk1": (4, 1, 4, 1, "USKTN", False), "fk2": (4, 1, 4, 2, "USKTN", False), "us": (4, 1, 4, 1, "US", False),
         "legacy": (4, 1, 4, 1, "U", True)}


# ---- stand-ins ---------------------------------------------------------------------------------------------------------------------------

class Header(dict):
    def __init__(self, unit, comment):
        super().__init__(UNIT=unit)
        self.comments = {"UNIT": comment}


class HDU:
    def __init__(self, data, header=None):
        self.data, self.header = data, header


class Cfg:
    pad_sides = "auto"

    def __init__(self, text=None, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class Timer:
    def __call__(self):
        return 0.0


LOG = []   # the calls of the loop, in order
SUMS = []  # the arguments of compress_map, in order


def reference_code():
    ref = os.environ["PYIMCOM_REFERENCE"]
    spec = importlib.util.spec_from_file_location("pyimcom_helper", os.path.join(ref, "diagnostics", "outimage_utils", "helper.py"))
    helper = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(helper)

    def methods(path, cls_name, names):
        tree = ast.parse(open(os.path.join(ref, path)).read(), filename=path)
        cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name)
        cls.body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(n.name for n in cls.body) == sorted(names)
        cls.bases, cls.keywords, cls.decorator_list = [], [], []
        return cls

    fits = types.SimpleNamespace(Header=None, ImageHDU=None)
    coadd = {"np": np, "fits": fits}
    exec(compile(ast.Module(body=[methods("coadd.py", "OutStamp", ["trapezoid"]), methods("coadd.py", "Block", ["compress_map"])], type_ignores=[]),
                 "coadd.py", "exec"), coadd)
    compress_map = coadd["Block"].compress_map

    class Block:
        @staticmethod
        def compress_map(map_, coef, dtype):
            SUMS.append(np.array(map_))
            return compress_map(map_, coef, dtype)

    ns = {"np": np, "Config": Cfg, "HDU_to_bels": helper.HDU_to_bels, "OutStamp": coadd["OutStamp"], "Block": Block, "Timer": Timer}
    exec(compile(ast.Module(body=[methods("analysis.py", "OutImage", ["_update_hdu_data", "get_output_map"]),
                                  methods("analysis.py", "Mosaic", ["share_padding_stamps"])], type_ignores=[]), "analysis.py", "exec"), ns)

    class OutImage(ns["OutImage"]):
        def __init__(self, key, block, cfg):
            self.key, self.cfg = key, cfg
            self.hdu_names = ["PRIMARY", "CONFIG", "INDATA", "INWEIGHT", "INWTFLAT"] + list(block["maps"])
            obsid, sca = [np.array(v, dtype=np.int64) for v in zip(*block["idscas"])]
            self.hdu_list = {"PRIMARY": HDU(block["primary"]), "CONFIG": HDU({"text": np.array(["#"])}), "INDATA": HDU({"obsid": obsid, "sca": sca}),
                             "INWEIGHT": HDU(block["inweight"]), "INWTFLAT": HDU(PR.inwtflat(block["inweight"]).copy())}
            for name, (codes, unit, comment) in block["maps"].items():
                self.hdu_list[name] = HDU(codes, Header(unit, comment))

        def _load_or_save_hdu_list(self, load_mode=True, save_file=False, auto_to_all=False):
            if load_mode or save_file:
                LOG.append(["load" if load_mode else "save", self.key[0], self.key[1]])

        def _update_hdu_data(self, neighbor, direction, add_mode=True):
            LOG.append(["update", list(self.key), list(neighbor.key), direction, bool(add_mode)])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # (the legacy-sign warning)
                super()._update_hdu_data(neighbor, direction, add_mode)

        def block(self):
            h = self.hdu_list
            assert np.array_equal(h["INWTFLAT"].data, PR.inwtflat(h["INWEIGHT"].data))  # 490-493
            return {"primary": h["PRIMARY"].data, "inweight": h["INWEIGHT"].data, "maps": {k: h[k].data for k in self.hdu_names[5:]}}

    return helper, OutImage, ns["Mosaic"]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------

def synthetic_block(seed, n_out, nlayer, n1P, n2, idscas, outmaps, legacy=False):
    """One block file's arrays.  Maps: 4 x 4 tiles in turn of random codes across the range, the floor code (uncovered area), the saturated
    code, random codes of a narrow band, the floor code again and one middle code, so that every strip meets all of them; big-endian int16
    as a FITS reader delivers it.  PRIMARY: layer 0 normal draws (eighths for the second output PSF), layer 1 small integers with zeros
    and negatives, layer 2 quarters.  (Runs and coarse values keep the compressed fixture small.)"""
    rng = np.random.default_rng(seed)
    N = n1P * n2
    primary = rng.standard_normal((n_out, nlayer, N, N)).astype(np.float32)
    if nlayer > 1:
        primary[:, 1] = rng.integers(-2, 3, (n_out, N, N)).astype(np.float32)
    if nlayer > 2:
        primary[:, 2] = (rng.integers(-3, 4, (n_out, N, N)) / np.float32(4)).astype(np.float32)
    primary[1:, 0] = (rng.integers(-8, 9, (n_out - 1, N, N)) / np.float32(8)).astype(np.float32)
    inweight = (rng.integers(0, 64, (n_out, len(idscas), n1P, n1P)) / np.float32(64)).astype(np.float32)
    ty, tx = np.indices((N, N)) // 4
    kind = (ty + 3 * tx + seed) % 8
    maps = {}
    for name, (letter, coef, dtype, unit, comment) in PR.MAPS.items():
        if letter not in outmaps:
            continue
        lo, hi = PR.code_range(dtype)
        floor, top = (lo, hi) if coef > 0 else (hi, lo)
        codes = rng.integers(lo, hi + 1, (n_out, N, N))
        band = rng.integers(-300, 300, (n_out, N, N)) + (lo + hi) // 2
        codes = np.where((kind == 1) | (kind == 4) | (kind == 6), floor, np.where((kind == 2) | (kind == 7), top, np.where(kind == 3, band, np.where(kind == 5, (lo + hi) // 2 + 77, codes))))
        codes = codes.astype(dtype)
        if legacy:
            unit = unit.lstrip("-")  # "0.2mB" with the comment "-5000*log10(U/C)"
        maps[name] = [codes.astype(">i2") if np.dtype(dtype) == np.int16 else codes, unit, comment]
    return {"primary": primary, "inweight": inweight, "idscas": list(idscas), "maps": maps}


def mosaic_inputs():
    m = MOSAIC
    blocks = [[synthetic_block(200 + 3 * iby + ibx, m["n_out"], m["nlayer"], m["n1P"], m["n2"], IDSCAS[(iby, ibx)], m["outmaps"]) for ibx in range(3)] for iby in range(3)]
    # (rows 10 .. 21 are left alone by the vertical pass)  the strip of (1, 1) that the replace call "left" overwrites from (1, 0): the neighbour's -0.0 arrives as +0.0 (mine * False = +0.0 is
    # added), and where mine holds inf the result is NaN
    blocks[1][1]["primary"][0, 0, 12, 1] = 1.5
    blocks[1][0]["primary"][0, 0, 12, 32 - 16 + 1] = -0.0
    blocks[1][1]["primary"][1, 0, 13, 2] = np.inf
    # ... and in the strip of (1, 0) that the add call "right" reads from (1, 1) and adds to: -0.0 + -0.0, and inf passed on
    blocks[1][0]["primary"][0, 0, 14, 32 - 10 + 3] = -0.0
    blocks[1][1]["primary"][0, 0, 14, 8 - 2 + 3] = -0.0
    blocks[1][1]["primary"][1, 2, 15, 8 - 2 + 4] = -np.inf
    return blocks


def pair_inputs(name):
    n2, pad, n1P, fk, outmaps, legacy = PAIRS[name]
    k = sorted(PAIRS).index(name)
    a = synthetic_block(300 + 2 * k, 2, 2, n1P, n2, [(1, 1), (2, 2), (3, 3)], outmaps, legacy)
    b = synthetic_block(301 + 2 * k, 2, 2, n1P, n2, [(3, 3), (4, 4), (1, 1), (3, 3)], outmaps, legacy)
    a["primary"][0, 0, 3, 2], a["primary"][0, 0, 12, 13], a["primary"][0, 1, 2, 3] = -0.0, np.inf, np.nan
    return a, b


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and a.dtype.newbyteorder("=") == b.dtype.newbyteorder("=") and np.array_equal(bits(a.astype(a.dtype.newbyteorder("="))),
                                                                                                             bits(b.astype(b.dtype.newbyteorder("="))))


def at(direction, s):
    return np.s_[..., :, s] if direction in ("left", "right") else np.s_[..., s, :]


def encode_differences(sums, add_mode, names, coefs, dtypes, stats):
    """The reference's encode against the device's formula on the same sums: per map strip the share of pixels that differ."""
    for name, s in zip(names, sums):
        ref, dev = PR.compress(s, coefs[name], dtypes[name]), PR.compress_device(s, coefs[name], dtypes[name])
        d = np.abs(ref.astype(np.int64) - dev.astype(np.int64))
        assert d.max() <= 1, f"{name}: the two encodes differ by {d.max()} counts"
        share = float(np.mean(d != 0))
        if add_mode:
            assert share <= CAP, f"{name}: {share:.4f} of an add strip differs"
            stats["add_strips"] += 1
            stats["add_pixels"] += d.size
            stats["add_differing"] += int(np.sum(d != 0))
            stats["add_worst_share"] = max(stats["add_worst_share"], share)
        else:
            assert share == 0.0, f"{name}: a replace strip differs"


def compute():
    helper, OutImage, Mosaic = reference_code()
    out, meta = {}, {"mosaic": dict(MOSAIC), "pairs": {}, "numpy": np.__version__, "cap": CAP}
    stats = {"add_strips": 0, "add_pixels": 0, "add_differing": 0, "add_worst_share": 0.0}
    coefs = {k: v[1] for k, v in PR.MAPS.items()}
    dtypes = {k: v[2] for k, v in PR.MAPS.items()}

    def store(prefix, block, strip=None):
        pick = (lambda a, s: a) if strip is None else (lambda a, s: np.ascontiguousarray(a[at(strip[0], s)]))
        out[prefix + "_primary"] = pick(block["primary"], strip and strip[1])
        out[prefix + "_inweight"] = pick(block["inweight"], strip and strip[2])
        for name, m in block["maps"].items():
            out[f"{prefix}_{name}"] = pick(m[0] if isinstance(m, list) else m, strip and strip[1])

    def forced_settings():
        """zero_floor settings that reproduce zero_floor=None on this numpy, per unit: (True matches, False matches)."""
        res = {}
        for name, (letter, coef, dtype, unit, comment) in PR.MAPS.items():
            lo, hi = PR.code_range(dtype)
            codes = np.arange(lo, hi + 1).astype(dtype)
            auto = PR.decode(codes, unit, comment)
            res[name] = [bool(same(auto, PR.decode(codes, unit, comment, True))), bool(same(auto, PR.decode(codes, unit, comment, False)))]
            hdu = HDU(codes, Header(unit, comment))
            assert 1.0 / helper.HDU_to_bels(hdu) == 1.0 / PR.unit_to_bels(unit, comment)
        return res

    meta["floor_rule"] = forced_settings()
    meta["decode_coef"] = {name: repr(1.0 / PR.unit_to_bels(v[3], v[4])) for name, v in PR.MAPS.items()}
    meta["units"] = {name: [v[3], v[4]] for name, v in PR.MAPS.items()}

    # ---- the mosaic case: the full loop
    m = MOSAIC
    blocks = mosaic_inputs()
    meta["mosaic"]["idscas"] = {f"{y},{x}": [list(p) for p in v] for (y, x), v in IDSCAS.items()}
    for iby in range(3):
        for ibx in range(3):
            store(f"mosaic_in_{iby}_{ibx}", blocks[iby][ibx])
    cfg = Cfg(NsideP=m["n1P"] * m["n2"], postage_pad=m["postage_pad"], n2=m["n2"], n1P=m["n1P"], fade_kernel=m["fk"], nblock=m["nblock"])
    mosaic = Mosaic()
    mosaic.cfg = cfg
    mosaic.outimages = [[OutImage((iby, ibx), PR.copy_block(blocks[iby][ibx]), cfg) for ibx in range(3)] for iby in range(3)]
    del LOG[:], SUMS[:]
    with contextlib.redirect_stdout(io.StringIO()):
        mosaic.share_padding_stamps()
    assert LOG == [list(s[:1]) + [list(v) if isinstance(v, tuple) else v for v in s[1:]] for s in PR.share_order(3)], "the restatement's order differs"
    meta["mosaic"]["order"] = list(LOG)
    names = list(blocks[0][0]["maps"])
    updates = [s for s in LOG if s[0] == "update"]
    assert len(SUMS) == len(updates) * len(names)
    for setting in (None,) + tuple(z for z in (True, False) if all(meta["floor_rule"][n][0 if z else 1] for n in names)):
        mine = [[PR.copy_block(blocks[iby][ibx]) for ibx in range(3)] for iby in range(3)]
        k = 0
        for step in PR.share_order(3):
            if step[0] != "update":
                continue
            (ay, ax), (by, bx) = step[1], step[2]
            sums = PR.update(mine[ay][ax], mine[by][bx], step[3], step[4], m["n2"], m["postage_pad"], m["fk"], setting)
            for name in names:
                assert same(sums[name], SUMS[k]), (setting, step, name)
                k += 1
        for iby in range(3):
            for ibx in range(3):
                got, want = mine[iby][ibx], mosaic.outimages[iby][ibx].block()
                assert same(got["primary"], want["primary"]) and same(got["inweight"], want["inweight"]), (setting, iby, ibx)
                assert all(same(got["maps"][n][0], want["maps"][n]) for n in names), (setting, iby, ibx)
    for iby in range(3):
        for ibx in range(3):
            store(f"mosaic_out_{iby}_{ibx}", mosaic.outimages[iby][ibx].block())
    for k, step in enumerate(updates):
        encode_differences(SUMS[k * len(names):(k + 1) * len(names)], step[4], names, coefs, dtypes, stats)
        if step[1] == [1, 1]:  # the centre block's four updates, one per combination the loop uses (the restatement gave all 24)
            for j, name in enumerate(names):
                out[f"mosaic_sums_{step[3]}_{name}"] = SUMS[k * len(names) + j]

    # ---- the pair cases: eight calls each, from the same two blocks
    for pname in sorted(PAIRS):
        n2, pad, n1P, fk, outmaps, legacy = PAIRS[pname]
        a, b = pair_inputs(pname)
        store(f"pair_{pname}_mine", a)
        store(f"pair_{pname}_theirs", b)
        names = list(a["maps"])
        meta["pairs"][pname] = {"n2": n2, "postage_pad": pad, "n1P": n1P, "fk": fk, "maps": {n: [a["maps"][n][1], a["maps"][n][2]] for n in names},
                                "mine_idscas": [list(p) for p in a["idscas"]], "theirs_idscas": [list(p) for p in b["idscas"]], "pairs": [list(p) for p in PR.pairs(a["idscas"], b["idscas"])]}
        cfg = Cfg(NsideP=n1P * n2, postage_pad=pad, n2=n2, n1P=n1P, fade_kernel=fk)
        stacked = {}  # array name -> my strip after each of the eight calls, flattened (the strips of rows and of columns differ in shape)
        meta["pairs"][pname]["calls"] = [[d, bool(m)] for d in PR.DIRECTIONS for m in (True, False)]
        for direction in PR.DIRECTIONS:
            for add_mode in (True, False):
                mine, theirs = OutImage((0, 0), PR.copy_block(a), cfg), OutImage((0, 1), PR.copy_block(b), cfg)
                del SUMS[:]
                mine._update_hdu_data(theirs, direction, add_mode)
                got, ur = mine.block(), theirs.block()
                assert same(ur["primary"], b["primary"]) and same(ur["inweight"], b["inweight"]) and all(same(ur["maps"][n], b["maps"][n][0]) for n in names)
                my, _ = PR.strips(direction, n1P * n2, pad * n2, fk)
                wmy, _ = PR.strips(direction, n1P, pad, 0)
                outside = np.ones(n1P * n2, dtype=bool)
                outside[my] = False
                assert same(got["primary"][at(direction, outside)], a["primary"][at(direction, outside)])
                assert all(same(got["maps"][n][at(direction, outside)], a["maps"][n][0][at(direction, outside)]) for n in names)
                case = f"pair_{pname}_{direction}_{'add' if add_mode else 'replace'}"
                stacked.setdefault("primary", []).append(got["primary"][at(direction, my)].ravel())
                stacked.setdefault("inweight", []).append(got["inweight"][at(direction, wmy)].ravel())
                for n in names:
                    stacked.setdefault(n, []).append(got["maps"][n][at(direction, my)].ravel())
                    stacked.setdefault("sums_" + n, []).append(SUMS[names.index(n)].ravel())
                for setting in (None, True, False):
                    rm, rt = PR.copy_block(a), PR.copy_block(b)
                    sums = PR.update(rm, rt, direction, add_mode, n2, pad, fk, setting)
                    matches_auto = setting is None or all(meta["floor_rule"][n][0 if setting else 1] for n in names)
                    if matches_auto:
                        assert same(rm["primary"], got["primary"]) and same(rm["inweight"], got["inweight"]), case
                        assert all(same(rm["maps"][n][0], got["maps"][n]) and same(sums[n], SUMS[j]) for j, n in enumerate(names)), (case, setting)
                encode_differences(SUMS, add_mode, names, coefs, dtypes, stats)
                if not add_mode:  # decode then encode returns the code: my strip holds the neighbour's codes
                    _, ur_s = PR.strips(direction, n1P * n2, pad * n2, fk)
                    assert all(np.array_equal(got["maps"][n][at(direction, my)], b["maps"][n][0][at(direction, ur_s)]) for n in names), case
        for key, rows in stacked.items():
            out[f"pair_{pname}_out_{key}"] = np.stack(rows)
    stats["add_share"] = stats["add_differing"] / max(stats["add_pixels"], 1)
    meta["encode"] = stats
    out["meta"] = np.array(json.dumps(meta))
    return out, meta


if __name__ == "__main__":
    arrays, meta = compute()
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    assert size < 495_000, size
    print(OUT, size, "bytes;", json.dumps(meta["encode"]), json.dumps(meta["floor_rule"]), json.dumps(meta["decode_coef"]))
