"""The radix front end at the edges of its payload pass and with 16-bit tile-sort keys (csrc/binning.hip,
csrc/scan_sort.hip) — needs an MI355X.

payload_kernel maps a grid of ceil(R / 256) blocks onto the sorted instance list and writes every instance's record, packed
word and range boundaries.  Whatever the block count — one single block, below 8, 1 or 7 beyond a multiple of 8 (the
hardware deals blocks to its 8 XCDs in turn; a mapping of blocks to XCD bands was measured and rejected, DESIGN §3.1, and
any such mapping has to pass here), 64 and more — every instance must be written exactly once: the radix run then equals
the binned front end (which never launches payload_kernel) in every list and bit of the forward state, and the CPU oracle.

The tile sort moves uint16_t keys when the window's (view, tile) ids fit 16 bits and the sort takes its histogram / scan /
scatter form (more than 1 048 576 instances); the last pass widens them into the uint32_t tile list.  Checked at the
smallest such R with two passes and with one (the only pass is the widening one), and on both sides of the 16-bit boundary
of a window of 8 views, where 17 bits keep the 32-bit path.

Every case asserts its own premise (block counts and R from the oracle or the run), so a change of the synthetic scenes
cannot silently move a case off the path it is there for.
"""
import functools

import pytest
import torch

from splatloc_amd import _native
from splatloc_amd.synthetic import make_scene
from tests.helpers import HipRun, oracle_backward, oracle_forward
from tests.test_gpu_binsort import _state_equal
from tests.test_gpu_parity import _check_backward, _check_forward

pytestmark = pytest.mark.gpu

ONE_SWEEP_MAX = 1 << 20     # sorts up to this many keys take the one-sweep form (scan_sort.hip: sweep_items)


@pytest.fixture(autouse=True)
def _restore_front_end():
    yield
    _native.set_front_end(-1)
    _native.check(_native.load().splatraster_debug_set_payload_stream_min(-1), "payload_stream_min")


def _blocks(R):
    return (R + 255) // 256


# name -> (scene, what its payload grid of ceil(R / 256) blocks must look like)
GRIDS = {
    "one_block": (lambda: make_scene(200, 17, 9, 4, 117, scale_median=0.08), lambda nb: nb == 1),
    "below_8": (lambda: make_scene(500, 17, 9, 4, 117, scale_median=0.08), lambda nb: 1 < nb < 8),
    "seven_blocks": (lambda: make_scene(1400, 17, 9, 4, 117, scale_median=0.08), lambda nb: nb == 7),
    "remainder_7": (lambda: make_scene(2740, 333, 201, 35, 22, scale_median=0.03), lambda nb: nb > 8 and nb % 8 == 7),
    "remainder_1": (lambda: make_scene(3080, 333, 201, 35, 22, scale_median=0.03), lambda nb: nb >= 64 and nb % 8 == 1),
    "many_blocks": (lambda: make_scene(10_000, 640, 480, 3, 0, scale_median=0.02), lambda nb: nb >= 64 and nb % 8 not in (0, 1, 7)),
}


@functools.lru_cache(maxsize=None)
def _grid_case(name):
    sc = GRIDS[name][0]()
    return sc, oracle_forward(sc)


def _radix_equals_binned_and_oracle(sc, f, backward=False):
    _native.set_front_end(0)
    radix = HipRun(sc, backward=backward)
    _native.set_front_end(1)
    binned = HipRun(sc, backward=False)
    _state_equal(radix, binned)
    _check_forward(radix, f, sc)
    return radix


@pytest.mark.parametrize("name", list(GRIDS))
def test_every_instance_is_written_once_whatever_the_block_count(name):
    sc, f = _grid_case(name)
    nb = _blocks(int(f["num_rendered"]))
    assert GRIDS[name][1](nb), (name, int(f["num_rendered"]), nb)
    _radix_equals_binned_and_oracle(sc, f)


@pytest.mark.parametrize("name", ["one_block", "remainder_7", "remainder_1"])
def test_streaming_store_instantiation_writes_the_same_payload(name):
    sc, f = _grid_case(name)
    assert GRIDS[name][1](_blocks(int(f["num_rendered"])))
    _native.check(_native.load().splatraster_debug_set_payload_stream_min(0), "payload_stream_min")
    _radix_equals_binned_and_oracle(sc, f)


@pytest.mark.parametrize("cfg,tiles_at_most_256", [
    (dict(P=12_000, W=640, H=480, C=3, seed=5, scale_median=0.12), False),     # 1200 tiles: 11 bits, two passes
    (dict(P=20_000, W=256, H=256, C=3, seed=26, scale_median=0.3), True),      # 256 tiles: 8 bits, the only pass widens
])
def test_sixteen_bit_keys_through_the_three_kernel_sort(cfg, tiles_at_most_256):
    sc = make_scene(**cfg)
    f = oracle_forward(sc)
    R = int(f["num_rendered"])
    tiles = ((cfg["W"] + 15) // 16) * ((cfg["H"] + 15) // 16)
    assert (tiles <= 256) == tiles_at_most_256
    assert R > ONE_SWEEP_MAX, R                      # the histogram / scan / scatter form
    if not tiles_at_most_256:
        assert R <= 2 * ONE_SWEEP_MAX, R             # ... at the smallest size that takes it
    radix = _radix_equals_binned_and_oracle(sc, f, backward=True)
    _check_backward(radix, oracle_backward(f, sc))


@pytest.mark.parametrize("W,lists,bits", [(1920, 65_280, 16), (1936, 65_824, 17)])
def test_window_on_both_sides_of_the_sixteen_bit_boundary(W, lists, bits):
    """8 views of 1920 x 1088 are 65 280 (view, tile) lists, the last ids use all 16 bits; 8 views of 1936 x 1088 are 65 824:
    17 bits, three passes of 32-bit keys.  Both windows hold more than 1 Mi instances (the per-view calls they are compared
    with stay below that and sort 32-bit keys in the one-sweep form), and equal the per-view calls bit for bit."""
    from tests.test_gpu_window import _compare
    V, H = 8, 1088
    assert V * ((W + 15) // 16) * ((H + 15) // 16) == lists and (lists - 1).bit_length() == bits
    _native.set_front_end(0)
    views, Lw, outs_w, m2_w = _compare(make_scene(500, W, H, 3, 421, scale_median=0.1), V)
    per_view = [int(r) for r in outs_w[0][0].grad_fn.R]
    assert len(per_view) == V and sum(per_view) > ONE_SWEEP_MAX, per_view
    assert max(per_view) <= ONE_SWEEP_MAX, per_view
    torch.cuda.synchronize()
