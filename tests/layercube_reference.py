"""numpy restatement of the input-layer cube (reference src/pyimcom/layer.py:1252-1492, the loop of ``get_all_data``), written against the
interface of ``pyimcom_amd.layers.build_cube`` -- in-memory ``sources``, ``grid_image`` and ``galsim_layers`` -- so that the same inputs drive
the restatement (tests/test_layercube_host.py, against the golden cubes the reference itself produced) and the device
(tests/test_gpu_layercube.py).  Plain numpy >= 2 on the host: the arithmetic is whatever numpy does with the arrays as they come."""

import json
import os
import re
import warnings

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layercube.npz")


def load_golden():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["meta"]))


def bits(a):
    """float32 bit patterns with every NaN as one."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def place(data, nside, origin=(0, 0), flip=0, subtract=None, scale=None):
    """One plane as the reference forms it: assign the window (minus the sky) to a float32 plane, reverse the plane, multiply it."""
    data = np.asarray(data)
    plane = np.zeros((nside, nside), dtype=np.float32)
    win = data[origin[0]:origin[0] + nside, origin[1]:origin[1] + nside]
    with np.errstate(all="ignore"):
        plane[:, :] = win if subtract is None else win - float(subtract)
        if flip == 1:
            plane[:, :] = plane[:, ::-1]
        elif flip == 2:
            plane[:, :] = plane[::-1, :]
        if scale is not None:
            plane *= float(scale)
    return plane


def pick(labels, label, filename):
    first = [j for j, lab in enumerate(labels) if lab == label]
    if not first:
        warnings.warn("WARNING: cannot find slice " + label + " in " + filename + ": continuing")
        return -1
    if len(first) > 1:
        warnings.warn("label " + label + " repeated in " + filename + ": using first instance")
    return first[0]


def noise_filename(case):
    ext = ".asdf" if case["informat"] == "L2_2506" else ".fits"
    return f"in/{case['informat']}_noise_{case['idsca'][0]}_{case['idsca'][1]}{ext}"


def make_sources(G, case, pick_slice=pick, convert=lambda a: a):
    """The ``sources`` callable of a golden case: the arrays in the byte order the case's files had, the sky beside them; for "noise" the
    slice chosen by ``pick_slice(labels, label, filename)`` with the warnings of a missing file or slice.  ``convert`` maps each array (to a
    device tensor, say)."""
    given = case["sources"]

    def sources(kind, label=None):
        if kind not in given:
            if kind == "noise":
                warnings.warn("WARNING: cannot find noise file: " + noise_filename(case) + ": continuing")
            return None
        key, extra = given[kind]
        if kind == "noise":
            j = pick_slice(extra, label, noise_filename(case))
            return None if j < 0 else convert(G[key][j])
        return convert(G[key]) if extra is None else (convert(G[key]), extra)

    return sources


def make_galsim(G, case):
    def provider(name, i):
        return G["gs"][case["galsim_plane"][str(i)]]

    return provider


def build_cube(case, sources, nside, grid_image=None, galsim_layers=None):
    """The loop of layer.py:1254-1492 in numpy, test by test in the reference's order."""
    informat, idsca, extrainput = case["informat"], case["idsca"], case["extrainput"]
    cube = np.zeros((len(extrainput), nside, nside), dtype=np.float32)
    flip = 0 if informat != "L2_2506" else (1 if idsca[1] % 3 == 0 else 2)

    def seed(q):
        return 1000000 * (18 * q + idsca[1]) + idsca[0]

    def split(got):
        return got if isinstance(got, tuple) else (got, None)

    if informat in ("dc2_imsim", "anlsim", "L2_2506"):
        data, sky = split(sources("sci"))
        if data is not None:
            cube[0] = place(data, nside, subtract=sky if informat != "L2_2506" else None)
    for i in range(1, len(extrainput)):
        name = extrainput[i]
        if name.casefold() == "truth" or name[:6].casefold() == "truth,":
            m = re.search(r"^truth,(.+)$", name, re.IGNORECASE)
            data, _ = split(sources("truth"))
            if data is not None:
                cube[i] = place(data, nside, flip=flip, scale=float(m.group(1)) if m else 1.0)
        m = re.search(r"^whitenoise(\d+)$", name, re.IGNORECASE)
        if m:
            cube[i] = np.random.default_rng(seed(int(m.group(1)))).normal(loc=0.0, scale=1.0, size=(nside, nside))
        if name.casefold() == "labnoise":
            data, _ = split(sources("labnoise"))
            if data is not None:
                origin = (0, 0) if np.shape(data) == (nside, nside) else (4, 4)
                cube[i] = place(data, nside, origin=origin, flip=flip)
        if name.casefold() == "skyerr":
            data, sky = split(sources("skyerr"))
            if data is not None:
                cube[i] = place(data, nside, subtract=sky)
        m = re.search(r"^cstar(\d+)$", name, re.IGNORECASE)
        if m:
            cube[i] = grid_image(int(m.group(1)))
        if re.search(r"^nstar(\d+),", name, re.IGNORECASE):
            res, args = int(re.search(r"^nstar(\d+),", name, re.IGNORECASE).group(1)), name.split(",")[1:]
            tot_int, bg, q = float(args[0]), float(args[1]), int(args[2])
            lam = grid_image(res) * tot_int + bg
            _lam = np.clip(lam, 0, None)
            cube[i] = np.random.default_rng(seed(q)).poisson(lam=_lam) - _lam + lam - bg
        for pattern in (r"^gsstar(\d+)$", r"^gstrstar(\d+)$", r"^gsfdstar(\d+),(.+)+$", r"^gsext(\d+)", r"^gsextchrom(\d+)"):
            if re.search(pattern, name, re.IGNORECASE):
                cube[i] = galsim_layers(name, i)
        m = re.search(r"^noise,(\S+)", name, re.IGNORECASE)
        if m:
            data, _ = split(sources("noise", str(m.group(1))))
            if data is not None:
                cube[i] = place(data, nside)
    return cube
