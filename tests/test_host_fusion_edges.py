"""Host side of the fusion stage's edge tests: the exact scenes' fixture (tests/golden/fusion_edges.npz, the reference's own f32
volumes) against the f32 restatement bit for bit, the stored tie counts recomputed, the vertex rule with its NaN behaviour on cases
worked out by hand, and every exact surface volume of tests/test_gpu_fusion_edges.py reaching the edge it is there for.  No GPU."""
import numpy as np
import pytest
import torch

from tests import fusion_reference as R

SEVEN = ("px_half", "py_half", "px_low", "px_high", "diff_trunc", "color_half", "z_zero")


@pytest.fixture(scope="module")
def fx():
    return R.edges_fixture()


def test_fixture_lists_the_scenes_and_kinds(fx):
    assert list(fx["scenes"]) == list(R.EDGE_SCENES) and list(fx["kinds"]) == list(R.TIE_KINDS) + ["updates"]
    assert set(R.EXACT_SCENES) <= set(R.EDGE_SCENES)
    assert {R.EDGE_SCENES[n]["feat_dim"] for n in R.EDGE_SCENES} >= {4, 8, 252}
    assert {R.EDGE_SCENES[n]["obs_weight"] for n in R.EDGE_SCENES} >= {0.5, 1.0, 2.0, 3.0}
    assert R.EDGE_W % 2 == 0 and R.EDGE_H % 2 == 1


@pytest.mark.parametrize("name", list(R.EDGE_SCENES))
def test_scene_is_exact_by_construction(name, fx):
    """rotations of 0 and +-1 entries with one entry per row and column, dyadic translations and grids with few bits: every
    product of the reference's matmul is exact and every sum representable; torch.inverse returns the analytic inverse exactly"""
    from splatloc_amd import fusion as F
    sc = R.edge_scene(name)
    for f in range(R.EDGE_FRAMES):
        rot = sc["poses"][f, :3, :3]
        assert set(np.unique(rot)) <= {-1.0, 0.0, 1.0} and (np.abs(rot).sum(axis=0) == 1).all() and (np.abs(rot).sum(axis=1) == 1).all()
        assert np.array_equal(torch.inverse(torch.from_numpy(sc["poses"][f]).float()).float().numpy(), sc["w2c"][f])
    assert np.array_equal(sc["w2c"], fx[f"{name}_w2c"])
    everything = np.concatenate([sc["poses"][:, :3, 3].ravel(), *sc["axes"], sc["K"].ravel(), [sc["sdf_trunc"]]])
    assert np.array_equal(everything * 1024, np.rint(everything * 1024)) and np.abs(everything).max() <= 8     # multiples of 2^-10
    assert any(rot is not R._I for rot, _ in R.EDGE_SCENES["perm"]["frames"])
    # the product builds the same axis tables from the same grid
    tables = F.axis_tables(torch.tensor(sc["dims"], dtype=torch.float64), torch.from_numpy(sc["origin"]), sc["voxel_size"])
    for t, a in zip(tables, sc["axes"]):
        assert np.array_equal(t.numpy(), a)
    assert np.float32(sc["margin"] * float(sc["voxel_size"])) == np.float32(sc["sdf_trunc"])
    # every depth value of the palette and a feature of 300 occur
    assert len(np.unique(sc["depth"][np.isfinite(sc["depth"])])) == len(R.EDGE_DEPTHS) - 2
    assert np.isnan(sc["depth"]).any() and np.isinf(sc["depth"]).any() and (sc["feat"] == 300).any()
    assert sc["color"].max() == 255 and sc["color"].min() == 0 and np.array_equal(sc["color"], np.rint(sc["color"]))


@pytest.mark.parametrize("name", list(R.EDGE_SCENES))
def test_restatement_equals_the_reference_bit_for_bit(name, fx):
    """all four volumes, every voxel: no mask (the share of excluded voxels is zero), and the tie counts as stored"""
    sc = R.edge_scene(name)
    counts = {}
    state = R.integrate_scene_f32(sc, counts=counts)
    assert np.array_equal(state["tsdf"], fx[f"{name}_tsdf"], equal_nan=True)
    assert np.array_equal(state["weight"], fx[f"{name}_weight"])
    assert np.array_equal(state["color"], fx[f"{name}_color"].astype(np.float32), equal_nan=True)
    assert np.array_equal(state["feat"].reshape(-1), fx[f"{name}_feat"].reshape(-1), equal_nan=True)
    assert fx[f"{name}_feat"].shape == (int(np.prod(sc["dims"])), sc["feat_dim"])
    stored = dict(zip(fx["kinds"].tolist(), fx[f"{name}_counts"].tolist()))
    assert counts == stored == R.tie_counts(name)
    assert all(stored[k] >= 100 for k in SEVEN), stored
    if name in R.EXACT_SCENES:
        assert stored["py_low"] >= 30 and stored["py_high"] >= 30
    w = fx[f"{name}_weight"]
    assert (w > 0).mean() > 0.4 and (w == 0).mean() > 0.1 and w.max() >= 4 * sc["obs_weight"]
    # the reproduced quirks are in the data: free space averaged in, features clamped at both ends
    assert ((fx[f"{name}_tsdf"] == 1) & (w > 0)).any() and fx[f"{name}_feat"].max() == 255 and fx[f"{name}_feat"].min() == 0


def test_both_outcomes_occur_at_each_image_boundary():
    """one voxel-frame each, by hand: K = (4, 4, 3.5, 2), image 9 x 8, camera at the origin looking along +z, depth 4 everywhere"""
    f32 = np.float32
    depth, color, feat = np.full((9, 8), 4, f32), np.full((9, 8, 3), 7, f32), np.ones((9, 8, 4), f32)
    K = np.array([[4, 0, 3.5], [0, 4, 2], [0, 0, 1]], f32)
    w2c = np.eye(4, dtype=f32)
    # x = -1, 1 at z = 1: pixel x = -0.5 -> -0.0 (in, pixel 0) and 7.5 -> 8 (out); y = 0.625, 1.625: 4.5 -> 4, 8.5 -> 8 (in)
    axes = [np.array([-1, 1, 1.25], f32), np.array([-0.625, 0.625, 1.625, 1.875], f32), np.array([1], f32)]
    st = R.integrate_f32(axes, R.fresh_state_f32(12, 4), depth, color, feat, K, w2c, 1.0, 0.375)
    w = st["weight"].reshape(3, 4)
    assert w.tolist() == [[1, 1, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]]      # y = 1.875: 9.5 -> 10, out; y = -0.625: -0.5 -> -0.0, in
    # depth_diff == -trunc is in, one ulp less is out; d = NaN, 0 and negative are out; inf is free space (dist 1)
    axes = [np.zeros(1, f32), np.zeros(1, f32), np.array([1], f32)]
    for d, weight, tsdf in ((0.625, 1, -1), (0.625 - 2.0 ** -10, 0, 1), (np.nan, 0, 1), (0.0, 0, 1), (-1.0, 0, 1), (np.inf, 1, 1),
                            (1.1875, 1, 0.5)):
        st = R.integrate_f32(axes, R.fresh_state_f32(1, 4), np.full((9, 8), d, f32), color, feat, K, w2c, 1.0, 0.375)
        assert (st["weight"][0], st["tsdf"][0]) == (weight, tsdf), d
    # z == 0 is behind; the colour means 7.5 and 6.5 round to 8 and 6 (half to even); a NaN feature stays NaN through the clamp
    st = R.integrate_f32([np.zeros(1, f32)] * 3, R.fresh_state_f32(1, 4), depth, color, feat, K, w2c, 1.0, 0.375)
    assert st["weight"][0] == 0
    feat[...] = np.nan
    for first, second, mean in ((7, 8, 8), (6, 7, 6)):
        st = R.fresh_state_f32(1, 4)
        for c in (first, second):
            R.integrate_f32(axes, st, depth, np.full((9, 8, 3), c, f32), feat, K, w2c, 1.0, 0.375)
        assert st["color"][0].tolist() == [mean] * 3 and st["weight"][0] == 2 and np.isnan(st["feat"]).all()


def _column(values, level):
    return R.surface_numpy(np.asarray(values, np.float32).reshape(1, 1, -1), level=level)


def test_vertex_rule_ties_by_hand():
    s = _column([-1, 1, -1, 1], 0.0)
    assert s["verts"][:, 2].tolist() == [0.5, 1.5, 2.5] and s["index"].tolist() == [0, 2, 2]       # half to even: 0, 2, 2
    assert s["edge"].tolist() == [[0, 2], [1, 2], [2, 2]]
    for shape, stride in (((4, 1, 1), 1), ((1, 4, 1), 1)):
        t = R.surface_numpy(np.asarray([-1, 1, -1, 1], np.float32).reshape(shape), level=0.0)
        assert t["index"].tolist() == [0, 2, 2] and t["verts"].max(axis=1).tolist() == [0.5, 1.5, 2.5]
    # quarter points are no ties
    s = _column([-1, 3, -1, -3, 1], 0.0)
    assert s["verts"][:, 2].tolist() == [0.25, 1.75, 3.75] and s["index"].tolist() == [0, 2, 4]


def test_vertex_rule_at_the_level_by_hand():
    # a == level: not below, so [0, -1] crosses at t = 0 / -1 = -0.0 (vertex at voxel 0) and [0, 1] does not cross
    s = _column([0, -1], 0.0)
    assert s["verts"][:, 2].tolist() == [0.0] and s["index"].tolist() == [0]
    assert _column([0, 1], 0.0)["verts"].shape == (0, 3)
    # b == level: [-1, 0] crosses at t = 1 (vertex at voxel 1)
    s = _column([-1, 0], 0.0)
    assert s["verts"][:, 2].tolist() == [1.0] and s["index"].tolist() == [1]
    # -0.0 is not below 0.0: it behaves as 0.0
    s = _column([-0.0, -1, -0.0, 1], 0.0)
    assert s["verts"][:, 2].tolist() == [0.0, 2.0] and s["index"].tolist() == [0, 2]
    # a level of its own: 0.5 + {-1, 0, 1} / 2
    s = _column([0.0, 0.5, 1.0, 0.5, 0.0], 0.5)
    assert s["verts"][:, 2].tolist() == [1.0, 3.0] and s["index"].tolist() == [1, 3]
    assert _column([0.5, 0.5, 0.5], 0.5)["verts"].shape == (0, 3)


def test_vertex_rule_with_nan_by_hand():
    # explicit level: [-1, NaN] crosses (-1 is below, NaN is not), its coordinate is NaN and its index the edge's own voxel;
    # [NaN, 1] does not cross, [NaN, -1] does (voxel 3 is below): own voxel again
    color = np.arange(15, dtype=np.float32).reshape(1, 1, 5, 3) + np.float32(0.99)
    feat = np.arange(20, dtype=np.float32).reshape(1, 1, 5, 4)
    s = R.surface_numpy(np.asarray([-1, np.nan, 1, np.nan, -1], np.float32).reshape(1, 1, 5), color, feat, level=0.0, voxel_size=0.5,
                        origin=[1.0, 2.0, 3.0])
    assert s["edge"].tolist() == [[0, 2], [3, 2]] and s["index"].tolist() == [0, 3]
    assert np.isnan(s["verts"][:, 2]).all() and np.isnan(s["points"][:, 2]).all()
    assert s["verts"][:, :2].tolist() == [[0, 0], [0, 0]] and s["points"][:, :2].tolist() == [[1, 2], [1, 2]]
    assert s["colors"].tolist() == [[0, 1, 2], [9, 10, 11]] and s["feats"].tolist() == [[0, 1, 2, 3], [12, 13, 14, 15]]
    # level None ignores NaN: min -1, max 3, level 1; the NaN edge crosses, [NaN, 3] does not, [3, -1] ties at 2.5 -> voxel 2
    s = _column([-1, np.nan, 3, -1], None)
    assert s["level"] == 1.0 and s["edge"].tolist() == [[0, 2], [2, 2]] and s["index"].tolist() == [0, 2]
    assert np.isnan(s["verts"][0, 2]) and s["verts"][1, 2] == 2.5
    # +-inf ends give NaN too: (0 + inf) / (1 + inf)
    s = _column([-np.inf, 1], 0.0)
    assert np.isnan(s["verts"][0, 2]) and s["index"].tolist() == [0]
    # NaN only: min = +inf, max = -inf, level NaN, nothing crosses
    s = _column([np.nan, np.nan, np.nan], None)
    assert np.isnan(s["level"]) and s["verts"].shape == (0, 3) and s["index"].shape == (0,)


@pytest.mark.parametrize("name", list(R.surface_cases()))
def test_every_surface_case_reaches_its_edge(name):
    case = R.surface_cases()[name]
    t = case["tsdf"]
    color, feat = R.surface_payload(t.shape, case["seed"])
    s = R.surface_numpy(t, color, feat, level=case["level"], voxel_size=0.125, origin=[0.5, -1.0, 2.0])
    v = s["verts"]
    assert v.shape[0] == case["count"] == s["index"].shape[0]
    with np.errstate(invalid="ignore"):
        tie = (v - np.floor(v) == 0.5).any(axis=1)
    nan = np.isnan(v).any(axis=1)
    assert tie.sum() >= case["ties"] and nan.sum() >= case["nans"]
    assert (case["count"] > 0) == (case["ties"] > 0) or name in ("all_nan", "one_voxel")
    if v.shape[0]:
        own = s["edge"][:, 0]
        step = np.array([t.shape[1] * t.shape[2], t.shape[2], 1])[s["edge"][:, 1]]
        assert ((s["index"] == own) | (s["index"] == own + step)).all() and (s["index"][nan] == own[nan]).all()
        assert np.array_equal(s["colors"], np.floor(color.reshape(-1, 3)[s["index"]]).astype(np.uint8))
        # a tie goes to the even end
        ijk = np.stack(np.unravel_index(s["index"], t.shape), axis=1)
        assert (ijk[tie, s["edge"][tie, 1]] % 2 == 0).all()
    if name.startswith("dyadic") or name.startswith("nan") or name.startswith("n_2"):
        # exact by construction: every coordinate is a multiple of 1/4, and both parities tie on every axis with more than 2 voxels
        ok = ~np.isnan(v)
        assert np.array_equal(v[ok] * 4, np.rint(v[ok] * 4))
        for ax in range(3):
            if t.shape[ax] > 2:
                lo = np.floor(v[tie & (s["edge"][:, 1] == ax), ax])
                assert (lo % 2 == 0).any() and (lo % 2 == 1).any(), ax
    if name == "dyadic_level_0":
        assert (t == 0).any() and np.signbit(t[t == 0]).any() and not np.signbit(t[t == 0]).all()
        assert (color - np.floor(color) > 0.98).any() and color.max() > 254.9
    if name == "checkerboard":
        assert np.array_equal(np.sort(v[np.arange(v.shape[0]), s["edge"][:, 1]] % 1), np.full(v.shape[0], 0.5, np.float32))
        assert 29000 < t.size < 31000


def test_nan_free_results_are_unchanged_by_the_nan_rules():
    """the extension only acts on NaN: on a NaN-free volume the index is rint(verts) and the level 0.5 * (min + max), as before"""
    t = R.dyadic_volume((6, 7, 9), 11)
    s = R.surface_numpy(t)
    assert s["level"] == np.float32(0.5) * (t.min() + t.max())
    r = np.rint(s["verts"]).astype(np.int64)
    assert np.array_equal(s["index"], (r[:, 0] * 7 + r[:, 1]) * 9 + r[:, 2])
