"""Sizes of the backward's gradient accumulator inside the `binning` buffer (host only: the sizing functions never touch the
GPU).  Layout rule (csrc/common.h, GaccLayout): a row of gacc_row_floats(C) columns = [C dL/dfeature | 7 moments | pad to 16];
for C >= 32 the first SH = C rounded down to a multiple of 16 columns are ONE row per Gaussian shared by the V views of a
window, the remaining PV = row - SH columns one row per (view, Gaussian); for C < 32, SH = 0.  So a single view's buffer is
what it always was, a window's is (V - 1) * P * SH floats smaller than V single views' accumulators."""
import pytest

ALIGN = 256
POSE_ACC_BYTES = 16 * 64 * 4 + 256


def _al(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def _moment_offset(C):
    return C if (C & 15) + 7 <= 16 else (C + 15) & ~15


def _row_floats(C):
    return (_moment_offset(C) + 7 + 15) & ~15


def _shared_floats(C):
    return (C & ~15) if C >= 32 else 0


def _gacc_bytes(P, V, C):
    SH = _shared_floats(C)
    return 4 * (P * SH + V * P * (_row_floats(C) - SH))


def _binning_bytes(lib, P, V, R, W, H, C, gacc_bytes):
    """the buffer's sections (csrc/capi.hip: bin_layout), each aligned to 256 bytes; frames here are too large for the split
    backward's checkpoints"""
    tiles = ((W + 15) // 16) * ((H + 15) // 16) * V
    assert 4 * tiles > 6144
    featp = P * ((C + 3) & ~3) * 4 if C % 4 else 16
    sort_tmp = lib.splatraster_sort_tmp_bytes(R) - 2 * _al(4 * R)    # (the exported size includes a key / value pair of its own)
    sections = [4 * R] * 4 + [8 * tiles, sort_tmp, 32 * R, 4 * R, featp, gacc_bytes, POSE_ACC_BYTES, 16,
                              4 * tiles, 4 * tiles]
    return sum(_al(s) for s in sections)


@pytest.fixture(scope="module")
def lib():
    from splatloc_amd import _native
    return _native.load()


@pytest.mark.parametrize("C", [4, 8, 32, 35, 40])
def test_single_view_buffer_is_unchanged(lib, C):
    P, R, W, H = 50_000, 400_000, 1920, 1080
    old_rows = 4 * P * _row_floats(C)          # one row of gacc_row_floats(C) floats per Gaussian, as before the shared table
    assert _gacc_bytes(P, 1, C) == old_rows
    assert lib.splatraster_binning_bytes(P, R, W, H, C) == _binning_bytes(lib, P, 1, R, W, H, C, old_rows)
    assert lib.splatraster_window_binning_bytes(P, 1, R, W, H, C) == lib.splatraster_binning_bytes(P, R, W, H, C)


def test_row_sizes_of_the_layout_rule():
    # C: (shared floats, per-view floats)
    want = {3: (0, 16), 4: (0, 16), 7: (0, 16), 8: (0, 16), 16: (0, 32), 31: (0, 48), 32: (32, 16), 35: (32, 16), 40: (32, 16),
            42: (32, 32), 47: (32, 32), 48: (48, 16), 64: (64, 16)}
    for C, (sh, pv) in want.items():
        assert (_shared_floats(C), _row_floats(C) - _shared_floats(C)) == (sh, pv), C
    assert _shared_floats(35) * 4 == 128 and (_row_floats(35) - _shared_floats(35)) * 4 == 64     # two lines + one line = 192 B


@pytest.mark.parametrize("C", [32, 35, 40, 48])
@pytest.mark.parametrize("V", [2, 5, 8])
def test_window_buffer_shares_the_colour_rows(lib, C, V):
    P, R, W, H = 50_000, 400_000, 1920, 1080
    got = lib.splatraster_window_binning_bytes(P, V, V * R, W, H, C)
    assert got == _binning_bytes(lib, P, V, V * R, W, H, C, _gacc_bytes(P, V, C))
    per_view_rows = _binning_bytes(lib, P, V, V * R, W, H, C, 4 * V * P * _row_floats(C))   # V single views' accumulators
    saved = (V - 1) * P * _shared_floats(C) * 4
    assert saved > 0 and abs((per_view_rows - got) - saved) < ALIGN


@pytest.mark.parametrize("C", [3, 4, 7, 8, 16])
def test_window_buffer_of_narrow_layouts_is_unchanged(lib, C):
    P, V, R, W, H = 50_000, 5, 400_000, 1920, 1080
    assert lib.splatraster_window_binning_bytes(P, V, V * R, W, H, C) == \
        _binning_bytes(lib, P, V, V * R, W, H, C, 4 * V * P * _row_floats(C))


def test_headline_window_accumulator_size(lib):
    """500k Gaussians, five views, C = 35: 480 MB of per-(view, Gaussian) rows -> 224 MB"""
    assert 4 * 5 * 500_000 * _row_floats(35) == 480_000_000
    assert _gacc_bytes(500_000, 5, 35) == 224_000_000
