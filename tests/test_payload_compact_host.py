"""Host side of the compact payload (csrc/binning.hip: payload_tile_kernel): what the sizing functions reserve for it, the debug
switch, and that neither moved anything older callers rely on.  No GPU: sizing and layout queries never touch one."""
import ctypes as C


def _al(n):
    return (n + 255) // 256 * 256


def test_image_buffer_holds_the_compact_plane_and_table():
    from splatloc_amd import _native
    lib = _native.load()
    for W, H, V in ((1920, 1080, 1), (1920, 1080, 5), (333, 201, 3), (17, 9, 8)):
        plane = _al(4 * W * H * V)
        tiles = V * ((W + 15) // 16) * ((H + 15) // 16)
        # final_T, n_contrib, n_contrib_c: 12 bytes per pixel; then cranges, uint32[2 * V * tiles]
        want = 3 * plane + _al(8 * tiles)
        assert lib.splatraster_window_image_bytes(W, H, V) == want
        if V == 1:
            assert lib.splatraster_image_bytes(W, H) == want
        L = _native.ImageLayout()
        assert lib.splatraster_get_window_image_layout(W, H, V, C.byref(L)) == 0
        assert (L.final_T, L.n_contrib, L.total) == (0, plane, want)      # the two planes older callers read did not move
    assert lib.splatraster_image_bytes(1920, 1080) >= 12 * 1920 * 1080


def test_binning_buffer_did_not_grow():
    """the table lives in the image buffer; the binning buffer's sections are the ones tests/test_accumulator_layout_sizes.py lists"""
    from splatloc_amd import _native
    lib = _native.load()
    P, R, W, H, Cn = 1000, 5000, 640, 480, 35
    B = _native.BinningLayout()
    assert lib.splatraster_get_binning_layout(P, R, W, H, Cn, C.byref(B)) == 0
    assert B.total == lib.splatraster_binning_bytes(P, R, W, H, Cn)
    assert B.point_list < B.tile_list < B.ranges == 4 * _al(4 * R)


def test_switch_is_exported_and_the_abi_version_is_20():
    from splatloc_amd import _native
    lib = _native.load()
    assert lib.splatraster_abi_version() == 20 == _native.ABI_VERSION
    assert "splatraster_debug_set_payload_compact" in _native.SYMBOLS
    for mode in (0, 1, -1):     # host-side switch: no device needed
        assert lib.splatraster_debug_set_payload_compact(mode) == 0
    _native.set_payload_compact(-1)
