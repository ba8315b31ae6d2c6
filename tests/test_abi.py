"""CPU-side checks of the boundary: the C-ABI library loads and exports every symbol that
include/imcom_hip.h declares; no compute calls here (no GPU in the build container)."""

import os
import re

import pytest

from tests.conftest import ROOT


def _declared():
    txt = open(os.path.join(ROOT, "include", "imcom_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(imcom_[A-Za-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported():
    import __graft_entry__ as g

    g.build()
    from pyimcom_amd import _lib

    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} declared in include/imcom_hip.h but not exported"
    assert set(names) == set(_lib.EXPORTED), set(names) ^ set(_lib.EXPORTED)
    assert _lib.lib.imcom_version() == 100


def test_no_gpu_fails_loudly():
    """Without a usable gfx950 device the context cannot be created and there is no fallback."""
    import pytest

    from pyimcom_amd import _lib

    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.ImcomError):
        _lib.Context(0)


def test_product_does_not_import_oracle():
    """Nothing under pyimcom_amd/ may import or call the oracle or the test-side checker (tests/parity.py)."""
    pkg = os.path.join(ROOT, "pyimcom_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and not dirpath.endswith(os.path.join("csrc", "tools")):  # tools/: developer scripts, not shipped code
                src = open(os.path.join(dirpath, f)).read()
                assert "from oracle" not in src and "import oracle" not in src and "tests" not in [w for l in src.splitlines()
                        if l.startswith(("from ", "import ")) for w in l.replace(".", " ").split()[1:2]], f


def test_package_import_asks_for_eight_hardware_queues():
    """The HIP runtime reads GPU_MAX_HW_QUEUES at its first call; the package sets 8 on import unless the caller has chosen (on the default
    of four, streams that share a queue wait for each other: profiles/r04_negative_results.txt item 18)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import os; import pyimcom_amd; print(os.environ['GPU_MAX_HW_QUEUES'])"
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    env["PYTHONPATH"] = root
    assert subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120).stdout.strip() == "8"
    env["GPU_MAX_HW_QUEUES"] = "6"
    assert subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120).stdout.strip() == "6"


@pytest.mark.gpu
def test_import_after_the_runtime_is_up_warns_and_changes_nothing():
    """A plug-in does not reconfigure its host's HIP runtime behind its back: when the device has been touched before the import
    (GPU_MAX_HW_QUEUES can no longer take effect) the package leaves the environment alone and says so once."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import os, warnings, torch; torch.zeros(1, device='cuda:0'); warnings.simplefilter('always');\n"
            "with warnings.catch_warnings(record=True) as w:\n    import pyimcom_amd\n"
            "print('GPU_MAX_HW_QUEUES' in os.environ, sum('GPU_MAX_HW_QUEUES' in str(x.message) for x in w))")
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    env["PYTHONPATH"] = root
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.stdout.split() == ["False", "1"], (out.stdout, out.stderr[-500:])


# One entry per source file whose entries take a context (pyimcom_amd/csrc/): a null context is refused before anything else
# is looked at, so every other argument may be zero / NULL and no device is touched.
NULL_CTX_ENTRIES = {
    "api.hip": "imcom_ctx_sync",
    "block.hip": "imcom_block_accumulate",
    "eigen.hip": "imcom_eigh",
    "ginterp.hip": "imcom_ginterp_matrix",
    "iter_empir.hip": "imcom_solve_iter",
    "partition.hip": "imcom_partition_pixels",
    "psf_overlap.hip": "imcom_psf_overlap",
    "psf_sample.hip": "imcom_sample_psf",
    "select.hip": "imcom_select_pixels",
    "inject.hip": "imcom_draw_stars",
    "imsubtract.hip": "imcom_imsub_canvas_add_f32",
    "splitpsf.hip": "imcom_splitpsf_tophat",
    "destripe.hip": "imcom_destripe_interp",
    "noisespec.hip": "imcom_noiseps_radial",
    "pcg64.hip": "imcom_cr_mask",
    "ziggurat.hip": "imcom_pcg64_normal",
    "noise1f.hip": "imcom_noise_1f",
    "objmask.hip": "imcom_mask_dilate",
    "quantiles.hip": "imcom_codehist",
    "i24.hip": "imcom_i24_decompress",
    "chol_solve.hip": "imcom_solve_chol_resident_end",
    "gemm_f64.hip": "imcom_ctx_mfma_probe",
    "interp.hip": "imcom_d5512_getw",
    "build_a.hip": "imcom_build_A",
    "la_kernels.hip": "imcom_trapezoid_f32",
    "starmom.hip": "imcom_star_moments",
    "wcs.hip": "imcom_wcs_pix2world",
}


def _null_argument(t):
    """0.0 for a ctypes float scalar, 0 for an integer scalar, None (a null pointer) for everything else."""
    import ctypes as C

    if t in (C.c_double, C.c_float):
        return 0.0
    if isinstance(t, type) and issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ":
        return 0
    return None


@pytest.mark.parametrize("source", sorted(NULL_CTX_ENTRIES))
def test_null_context_is_refused(source):
    from pyimcom_amd import _lib

    name = NULL_CTX_ENTRIES[source]
    args = [_null_argument(t) for t in _lib.SIGNATURES[name]]
    assert getattr(_lib.lib, name)(*args) == -1  # IMCOM_ERR_ARG
    assert "null context" in _lib.lib.imcom_last_error().decode()


def test_every_context_source_is_covered():
    """The table above names every source file that defines an entry taking a context."""
    csrc = os.path.join(ROOT, "pyimcom_amd", "csrc")
    have = set()
    for f in os.listdir(csrc):
        if f.endswith(".hip") and re.search(r'^(extern "C" )?int imcom_\w+\(imcom_ctx \*', open(os.path.join(csrc, f)).read(), re.M):
            have.add(f)
    assert have == set(NULL_CTX_ENTRIES), have ^ set(NULL_CTX_ENTRIES)


def test_launchers_header_declares_only_cross_file_calls():
    """launchers.h's first sentence as an assertion: every function it declares is defined in exactly one .hip and called from at
    least one other source file of csrc/ (what only its own file calls is static there and has no line in the header)."""
    csrc = os.path.join(ROOT, "pyimcom_amd", "csrc")

    def code(f):  # the file without its comments
        txt = open(os.path.join(csrc, f)).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))

    not_functions = {"int", "sizeof", "static_assert"}  # std::function<int(int)> and the like
    header = code("launchers.h")
    names = sorted(set(re.findall(r"\b([A-Za-z_]\w*)\s*\(", header)) - not_functions)
    assert len(names) >= 40, names
    sources = {f: code(f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and f != "launchers.h"}
    for name in names:
        # a definition: the name at the start of a declarator on a line that does not end the statement, followed by a body
        definition = re.compile(r"^[A-Za-z_][\w \t\*&:<>]*?\b%s\s*\([^;{}]*\)\s*(const\s*)?\{" % re.escape(name), re.M)
        defined = [f for f, txt in sources.items() if f.endswith(".hip") and definition.search(txt)]
        assert len(defined) == 1, f"{name}: defined in {defined}"
        assert not re.search(r"^static\b[^;{}]*\b%s\s*\(" % re.escape(name), sources[defined[0]], re.M), f"{name} is static in {defined[0]}"
        callers = [f for f, txt in sources.items() if f != defined[0] and re.search(r"\b%s\s*\(" % re.escape(name), txt)]
        assert callers, f"{name} (launchers.h) is called only from {defined[0]}: make it static there"
