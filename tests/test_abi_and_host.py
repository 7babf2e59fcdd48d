"""CPU-side checks: the C-ABI library loads and exports every symbol include/splatraster.h
declares; host-side mirror of the diff_gauss / simple_knn API (names, arguments, errors)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "splatraster.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(splat(?:raster|knn)_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_are_exported():
    from splatloc_amd import _native
    lib = _native.load()
    declared = _declared_symbols()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/splatraster.h but not exported"
    assert set(declared) == set(_native.SYMBOLS), "ctypes table and header disagree"
    assert os.path.dirname(_native.lib_path()).startswith(ROOT)   # in-tree .so


def test_host_only_entry_points():
    """Sizing / layout / error-string functions never touch the GPU."""
    from splatloc_amd import _native
    lib = _native.load()
    import re
    hdr = open(os.path.join(ROOT, "include", "splatraster.h")).read()
    declared_version = int(re.search(r"#define SPLATRASTER_ABI_VERSION (\d+)", hdr).group(1))
    assert lib.splatraster_abi_version() == declared_version == _native.ABI_VERSION
    assert lib.splatraster_poll_errors() == 0          # no device touched yet: nothing to report
    assert lib.splatraster_error_string(0) == b"ok" and lib.splatraster_error_string(1) == b"bad argument"
    g1, g2 = lib.splatraster_geometry_bytes(1000), lib.splatraster_geometry_bytes(500_000)
    assert 0 < g1 < g2 and g2 % 256 == 0
    b = lib.splatraster_binning_bytes(500_000, 4_000_000, 1920, 1080, 35)
    assert b >= 16 * 4_000_000
    assert lib.splatraster_image_bytes(1920, 1080) >= 8 * 1920 * 1080
    L = _native.GeometryLayout()
    assert lib.splatraster_get_geometry_layout(1000, C.byref(L)) == 0
    offs = [L.rec0, L.tiles_touched, L.depth_order, L.offsets, L.rgb, L.clamped]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and L.total == g1
    assert L.rec1 == L.rec0 + 16          # interleaved 32-byte records
    B = _native.BinningLayout()
    assert lib.splatraster_get_binning_layout(1000, 5000, 640, 480, 4, C.byref(B)) == 0
    assert B.total == lib.splatraster_binning_bytes(1000, 5000, 640, 480, 4)
    # narrow layouts (C <= 4) of small frames hold the forward's list checkpoints for the split backward:
    # 3 checkpoints x (C + 2) planes
    b8 = lib.splatraster_binning_bytes(1000, 5000, 640, 480, 8)
    assert B.total >= b8 - 1000 * 4 * 4 + 3 * (4 + 2) * 640 * 480 * 4 - 4096
    # C % 4 != 0 adds the 16-byte-aligned feature table
    assert lib.splatraster_binning_bytes(1000, 5000, 640, 480, 35) >= b8 + 1000 * (36 - 8) * 4 - 256
    assert lib.splatraster_get_geometry_layout(10, None) == 1           # BAD_ARG, no crash
    assert lib.splatknn_workspace_bytes(20_000) >= 20_000 * 12
    assert lib.splatraster_sort_tmp_bytes(1 << 20) > 8 * (1 << 20)


def test_bad_arguments_return_status_not_crash():
    from splatloc_amd import _native
    lib = _native.load()
    st = _native.Settings(480, 640, 1.0, 0.75, 1.0, 0, 0, 3, 3, 0, 0)
    R = C.c_int64(-1)
    # P > 0 with null pointers -> BAD_ARG before any HIP call
    rc = lib.splatraster_forward_geometry(C.byref(st), 10, None, None, None, None, None, None, None, None, None,
                                          None, None, C.byref(R), None)
    assert rc == 1 and R.value == 0
    bad = _native.Settings(0, 640, 1.0, 0.75, 1.0, 0, 0, 3, 3, 0, 0)
    assert lib.splatraster_forward_geometry(C.byref(bad), 0, *([None] * 11), C.byref(R), None) == 1
    assert lib.splatknn_dist2(-1, None, None, None, None) == 1
    assert lib.splatknn_dist2(0, None, None, None, None) == 0
    assert lib.splatraster_sort_pairs_u32(5, None, None, 8, None, None) == 1
    # the scan / sort test hooks: null pointers with n > 0, exclusive with a perm, a span_owner or in != out, span 0, a gathered
    # scan in place, and the uint16_t sort at a size or width that has no such form
    a, b = C.c_void_p(256), C.c_void_p(512)                             # never dereferenced: refused first
    scan = lib.splatraster_debug_scan_u32
    assert scan(-1, a, None, b, None, 0, None, 0, 0, a, None) == 1
    assert scan(5, None, None, b, None, 0, None, 0, 0, a, None) == 1
    assert scan(5, a, None, None, None, 0, None, 0, 0, a, None) == 1
    assert scan(5, a, None, b, None, 0, None, 0, 0, None, None) == 1
    assert scan(5, a, None, b, None, 1, None, 0, 0, a, None) == 1      # exclusive, in != out
    assert scan(5, a, b, a, None, 1, None, 0, 0, a, None) == 1         # exclusive with a perm
    assert scan(5, a, None, a, None, 1, b, 1024, 4, a, None) == 1      # exclusive with a span_owner
    assert scan(5, a, None, b, None, 0, b, 0, 4, a, None) == 1         # span 0
    assert scan(5, a, b, a, None, 0, None, 0, 0, a, None) == 1         # gathered and in place
    assert scan(0, None, None, None, None, 0, None, 0, 0, None, None) == 0
    k16 = lib.splatraster_debug_sort_pairs_k16
    assert k16(1_048_577, None, None, 8, None, None) == 1
    assert k16(1_048_577, a, b, 8, None, None) == 1
    assert k16(1_048_576, a, b, 8, a, None) == 1                        # one-sweep size: no uint16_t form
    assert k16(1_048_577, a, b, 17, a, None) == 1 and k16(1_048_577, a, b, 0, a, None) == 1 and k16(0, a, b, 8, a, None) == 1
    assert k16(-1, a, b, 8, a, None) == 1
    assert lib.splatraster_debug_sort_path(1_048_576, 8, 1) == -1 and lib.splatraster_debug_scan_path(-1) == -1
    # the §8f stages validate before any HIP call too
    N13, N19 = [None] * 13, [None] * 19
    assert lib.splatraster_activate_forward(0, 1, 0, 3, 0, *N13) == 0                   # P = 0: nothing to do
    assert lib.splatraster_activate_forward(10, 1, 0, 3, 0, *N13) == 1                  # null inputs
    assert lib.splatraster_activate_forward(10, 1, 4, 3, 0, *N13) == 3                  # SH degree 4: unsupported
    assert lib.splatraster_activate_forward(10, 1, 1, 3, 0, *N13) == 1                  # degree 1 needs 4 coefficients
    assert lib.splatraster_activate_forward(10, 1, 0, 2, 0, *N13) == 1                  # scaling columns must be 1 or 3
    assert lib.splatraster_activate_backward(10, 4, 1, 3, 1, *N19) == 1
    assert lib.splatraster_mapping_loss(0, *([None] * 6), C.c_float(0.01), *([None] * 7)) == 1
    assert lib.splatraster_mapping_loss(100, *([None] * 6), C.c_float(0.01), *([None] * 7)) == 1
    assert lib.splatraster_refinement_loss(3, 0, 8, C.c_float(0.2), *([None] * 6)) == 1
    assert lib.splatraster_densification_stats(-1, *([None] * 6)) == 1
    assert lib.splatraster_densification_stats(0, *([None] * 6)) == 0
    assert lib.splatraster_mapping_loss_workspace_bytes(640 * 480) > 0
    assert lib.splatraster_refinement_loss_workspace_bytes(3, 480, 640) >= 3 * 4 * 3 * 480 * 640
    assert lib.splatraster_timing_select(0) == 0 and lib.splatraster_timing_enable(0) == 0


def test_drop_in_module_names():
    import diff_gauss
    from diff_gauss import GaussianRasterizationSettings, GaussianRasterizer  # gaussian_renderer/__init__.py:4-7
    from simple_knn._C import distCUDA2                                        # gaussian_model.py:18
    assert diff_gauss.rasterize_gaussians is not None and callable(distCUDA2)
    assert GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug")
    assert issubclass(GaussianRasterizer, torch.nn.Module)


def _settings():
    from diff_gauss import GaussianRasterizationSettings
    return GaussianRasterizationSettings(48, 64, 1.0, 0.75, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                         torch.zeros(3), False, False)


def test_rasterizer_argument_validation():
    """exactly one of shs/colors_precomp and of (scales, rotations)/cov3D_precomp."""
    from diff_gauss import GaussianRasterizer
    r = GaussianRasterizer(raster_settings=_settings())
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=z(4, 3), means2D=z(4, 3), opacities=z(4, 1), shs=None, colors_precomp=None, scales=z(4, 3),
          rotations=z(4, 4))
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=z(4, 3), means2D=z(4, 3), opacities=z(4, 1), shs=z(4, 1, 3), colors_precomp=z(4, 3),
          scales=z(4, 3), rotations=z(4, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=z(4, 3), means2D=z(4, 3), opacities=z(4, 1), colors_precomp=z(4, 3))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=z(4, 3), means2D=z(4, 3), opacities=z(4, 1), colors_precomp=z(4, 3), scales=z(4, 3),
          rotations=z(4, 4), cov3D_precomp=z(4, 6))


def test_cpu_tensors_fail_loudly():
    """No CPU fallback: the product path refuses host tensors instead of computing elsewhere."""
    from diff_gauss import GaussianRasterizer
    from simple_knn._C import distCUDA2
    r = GaussianRasterizer(raster_settings=_settings())
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(means3D=z(4, 3), means2D=z(4, 3), opacities=z(4, 1), colors_precomp=z(4, 3), scales=z(4, 3),
          rotations=z(4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distCUDA2(z(10, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.markVisible(z(4, 3))


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under the product packages may reference it."""
    for pkg in ("splatloc_amd", "diff_gauss", "simple_knn"):
        for dp, _, files in os.walk(os.path.join(ROOT, pkg)):
            for f in files:
                if f.endswith((".py", ".hip", ".h")):
                    txt = open(os.path.join(dp, f)).read()
                    assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), os.path.join(dp, f)
                    assert "splat_oracle" not in txt and "liborc" not in txt, os.path.join(dp, f)


def test_concurrent_imports_after_a_source_change_build_once_and_all_load():
    """Every rank of a `torchrun --nproc-per-node N` job imports the package at the same moment.  With a stale manifest
    (= a source edit) they would all rebuild: the build holds an exclusive flock and installs the objects, the library
    and the manifest with atomic renames, so one process builds, the others wait and find everything up to date, and
    nobody dlopens a half-written ELF (round-2 advisor finding)."""
    import json
    import subprocess
    import sys
    from splatloc_amd import build
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    build.build()
    m = json.load(open(build.MANIFEST))
    m["knn.hip"] = "stale"                      # what a source edit looks like to up_to_date()
    json.dump(m, open(build.MANIFEST, "w"))
    code = ("from splatloc_amd import _native; lib = _native.load(); "
            "print('ok', lib.splatraster_abi_version())")
    procs = [subprocess.Popen([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for _ in range(4)]
    outs = [p.communicate() for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-400:] for o in outs]
    assert all(o[0].split() == ["ok", str(_abi())] for o in outs), outs
    assert build.up_to_date()


def _abi():
    from splatloc_amd import _native
    return _native.ABI_VERSION


def test_probe_patches_apply():
    """The timing probes live as patches beside the sources (tools/patches), not in the shipped translation
    units — and a patch nobody applies rots with the first kernel change (round 4 found two dead hunks).  Every patch must
    apply cleanly to the current tree (`patch -p1 --dry-run`; no fuzz, no rejects)."""
    import glob
    import shutil
    import subprocess
    if not shutil.which("patch"):
        pytest.skip("patch(1) not installed")
    patches = sorted(glob.glob(os.path.join(ROOT, "tools", "patches", "*.patch")))
    assert patches
    for p in patches:
        r = subprocess.run(["patch", "-p1", "--dry-run", "--fuzz=0", "-i", p], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0 and "FAILED" not in r.stdout and "fuzz" not in r.stdout, (p, r.stdout[-800:], r.stderr[-400:])


def test_profiles_readme_is_the_generated_one_and_describes_every_file():
    """profiles/README.md is GENERATED from the files it describes (tools/profiles_readme.py): the committed copy must equal a
    fresh rendering — round 5 replaced a profile and not the table — and no row may be "(undescribed)"."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("profiles_readme", os.path.join(ROOT, "tools", "profiles_readme.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = mod.render()
    with open(os.path.join(ROOT, "profiles", "README.md")) as f:
        committed = f.read()
    assert "(undescribed)" not in fresh, [ln[:60] for ln in fresh.splitlines() if "(undescribed)" in ln]
    assert fresh == committed, "profiles/README.md is stale: run `python tools/profiles_readme.py`"


def test_history_sections_are_numbered_once():
    import re
    with open(os.path.join(ROOT, "HISTORY.md")) as f:
        heads = re.findall(r"^## (\d+)\.", f.read(), flags=re.M)
    assert len(heads) == len(set(heads)), heads
