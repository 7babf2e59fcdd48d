"""The scenes of tests/test_gpu_dead_marks.py contain what they are there for — shown on the CPU, by the reference alone
(tests/dead_marks_reference.py over the oracle's forward): enough walked candidates without a contributing pixel, in every chunk
of one list and in the chunk in which a quadrant finishes, and the sets the GPU test asserts on are consistent."""
import numpy as np
import pytest

from tests.dead_marks_reference import SCENES, dead_mark_sets, occluder_scene, quadrant_finish_chunks
from tests.helpers import oracle_forward


def _sets(name, C=35):
    kw = SCENES[name]
    sc = occluder_scene(C, **kw)
    f = oracle_forward(sc)
    return sc, f, dead_mark_sets(f, kw["W"], kw["H"]), kw


@pytest.mark.parametrize("name", sorted(SCENES))
def test_sets_are_consistent(name):
    _, f, s, kw = _sets(name)
    assert not (s["must_mark"] & s["must_not"]).any()
    assert not (s["must_mark"] & s["contributes"]).any()
    assert not (s["must_not"] & ~s["contributes"]).any()          # the decided contributors are among the possible ones
    assert not (s["must_not"] & ~s["reach"]).any(), "a contributor without its reach bit: the restated mask is not conservative"
    assert not (s["must_not"] & ~s["walked"]).any()
    assert s["must_mark"].any() and s["must_not"].any()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_holds_dead_candidates_where_the_kernels_can_go_wrong(name):
    _, f, s, kw = _sets(name)
    W, H = kw["W"], kw["H"]
    gx = (W + 15) // 16
    t = (kw["oy"] // 16) * gx + kw["ox"] // 16
    lo, hi = (int(v) for v in f["ranges"][t])
    assert 140 <= hi - lo <= 200, hi - lo                          # one list of about 150 entries: three chunks
    walked = s["walked"]
    dead = walked & (s["must_mark"] | ~s["contributes"])          # in must-mark, or without a contributing pixel
    share = dead.sum() / walked.sum()
    print(f"{name}: list {hi - lo}, walked candidate-quadrants {walked.sum()}, dead {dead.sum()} ({100 * share:.1f} %), "
          f"must-mark {s['must_mark'].sum()}")
    assert share >= 0.05
    in_list = s["tile"] == t
    chunk = s["pos"] // 64
    for c, sel in ((0, chunk == 0), (1, chunk == 1), (2, chunk >= 2)):
        assert (dead[in_list & sel]).any(), f"no dead candidate in chunk {c} of the list"
        assert (s["must_mark"][in_list & sel]).any(), f"no must-mark entry in chunk {c} of the list"
    # inside the chunk in which a quadrant finishes: a dead candidate OF that quadrant, in front of its last contributor
    fin = quadrant_finish_chunks(f, W, H, t)
    assert any(c >= 0 and dead[in_list & (chunk == c), q].any() for q, c in enumerate(fin)), fin
    # occlusion: a candidate whose pixels all pass the alpha test somewhere but contribute nowhere
    occluded = walked & ~s["contributes"] & ~s["must_mark"]
    assert occluded.any()


def test_quadrants_outside_the_image_hold_no_set():
    for name in ("edge", "edge_row"):
        _, f, s, kw = _sets(name)
        W, H = kw["W"], kw["H"]
        gx = (W + 15) // 16
        for q in range(4):
            x0, y0 = kw["ox"] + 8 * (q & 1), kw["oy"] + 8 * (q >> 1)
            if x0 >= W or y0 >= H:
                t = (kw["oy"] // 16) * gx + kw["ox"] // 16
                for k in ("walked", "must_mark", "must_not"):
                    assert not s[k][s["tile"] == t, q].any(), (name, q, k)
