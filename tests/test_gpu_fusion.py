"""Feature-TSDF fusion on the MI355X: the device against the reference's volumes (tests/golden/fusion_*.npz) under the recorded
bars and masks, batches against single frames bit for bit, frames that must change nothing, the surface against the numpy rule on
the device's own volume, checkpoints, the decoder trained on the fused cloud, and one volume of office_0's size (22.9 GB)."""
import numpy as np
import pytest
import torch

from tests import fusion_reference as R

pytestmark = pytest.mark.gpu


def _volume(name, **kw):
    from splatloc_amd.fusion import TSDFVolume
    fx, cfg = R.fixture(name), R.SCENES[name]
    vol = TSDFVolume(torch.from_numpy(fx["voxel_dim"]), torch.from_numpy(fx["origin"]), cfg["voxel_size"], kw.pop("feat_dim", cfg["feat_dim"]),
                     margin=cfg["margin"], **kw)
    return vol, fx


def _frames(name, fx, feat_dim=None):
    color, feat = R.images(name)
    if feat_dim is not None and feat_dim != feat.shape[-1]:
        feat = np.random.default_rng(77).random((R.FRAMES, R.H, R.W, feat_dim), dtype=np.float32) - np.float32(0.4)
    cuda = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    return cuda(fx["depth"]), cuda(color), cuda(feat), torch.from_numpy(fx["K"]), torch.from_numpy(fx["poses"])


def _fused(name):
    vol, fx = _volume(name)
    vol.integrate_frames(*_frames(name, fx))
    return vol, fx


def _clone(vol):
    return [t.clone() for t in vol.get_volume()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(R.SCENES))
def test_device_against_the_reference_volumes(name):
    """Bars: 4 x the recorded max |reference f32 - float64 restatement| per quantity, against the reference's f32 result, on the
    decided voxels (and colour elements away from a tie); weight bit-exact.  Colour and features depend on the chosen pixel and the
    weights only: whether they are bit-equal is printed."""
    vol, fx = _fused(name)
    for t, k in zip(vol._axis, ("axis_x", "axis_y", "axis_z")):
        assert np.array_equal(t.cpu().numpy(), fx[k])
    N, C = int(np.prod(fx["dims"])), int(fx["feat_dim"])
    tsdf, color, weight, feat = (t.cpu().numpy() for t in vol.get_volume())
    tsdf, weight, color, feat = tsdf.reshape(N), weight.reshape(N), color.reshape(N, 3), feat.reshape(N, C)
    ok = ~fx["undecided"]
    col_ok = ok[:, None] & ~fx["tie"]
    s = fx["sample_idx"]
    featsum = feat.astype(np.float64).sum(axis=1)
    e_tsdf = np.abs(tsdf.astype(np.float64) - fx["tsdf"])[ok].max()
    e_col = np.abs(color.astype(np.float64) - fx["color"])[col_ok].max()
    e_feat = np.abs(feat[s].astype(np.float64) - fx["sample_feat"]).max()
    e_sum = np.abs(featsum - fx["featsum"])[ok].max()
    print(f"\n{name}: tsdf {e_tsdf:.3e} (bar {4 * fx['dev_tsdf']:.3e}), colour {e_col:.3e} (bar {4 * fx['dev_color']:.3e}), "
          f"feature rows {e_feat:.3e} (bar {4 * fx['dev_feat']:.3e}), channel sums {e_sum:.3e} (bar {4 * fx['dev_featsum']:.3e}); "
          f"bit-equal: tsdf {np.array_equal(tsdf[ok], fx['tsdf'][ok])}, colour {e_col == 0}, feature rows "
          f"{np.array_equal(feat[s], fx['sample_feat'])}, channel sums {np.array_equal(featsum[ok], fx['featsum'][ok])}; "
          f"undecided voxels that differ in weight: {int((weight != fx['weight'])[~ok].sum())} of {int((~ok).sum())}")
    assert np.array_equal(weight[ok], fx["weight"][ok])
    assert e_tsdf <= 4 * float(fx["dev_tsdf"])
    assert e_col <= 4 * float(fx["dev_color"])
    assert e_feat <= 4 * float(fx["dev_feat"])
    assert e_sum <= 4 * float(fx["dev_featsum"])
    assert (weight > 0).sum() > 0.1 * N


@pytest.mark.parametrize("name", list(R.SCENES))
def test_a_batch_is_bit_identical_to_single_frames(name):
    vol, fx = _volume(name)
    depth, color, feat, K, poses = _frames(name, fx)
    for f in range(R.FRAMES):
        vol.integrate(depth[f], color[f], feat[f], K, poses[f])
    singles = _clone(vol)
    vol.reset()
    vol.integrate_frames(depth, color, feat, K, poses)
    assert _same(singles, vol.get_volume())
    vol.reset()
    vol.integrate_frames(depth[:3], color[:3], feat[:3], K, poses[:3])
    vol.integrate_frames(depth[3:], color[3:], feat[3:], K, poses[3:])
    assert _same(singles, vol.get_volume())
    # more than 8 frames are chunked: 8 + 3 equals 11 singles
    vol.reset()
    idx = list(range(R.FRAMES)) + [1, 4, 6]
    vol.integrate_frames(depth[idx], color[idx], feat[idx], K, poses[idx])
    chunked = _clone(vol)
    vol.reset()
    for f in idx:
        vol.integrate(depth[f], color[f], feat[f], K, poses[f])
    assert _same(chunked, vol.get_volume())
    assert float(vol.get_volume()[2].max()) >= 2       # voxels seen by several frames: the running means were exercised


def test_reset_and_frames_that_change_nothing():
    vol, fx = _fused("c8")
    depth, color, feat, K, poses = _frames("c8", fx)
    before = _clone(vol)
    assert float(before[2].max()) > 0
    # an empty frame: all depth 0
    vol.integrate(torch.zeros_like(depth[0]), color[0], feat[0], K, poses[0])
    assert _same(before, vol.get_volume())
    # a camera outside the volume that looks away from it: every voxel is behind it
    away = torch.from_numpy(R.look_at([0.0, 0.0, 2.0], [0.0, 0.3, 5.0]).astype(np.float32))
    vol.integrate(torch.full_like(depth[0], 1.5), color[0], feat[0], K, away)
    assert _same(before, vol.get_volume())
    # the same camera turned round does change it
    back = torch.from_numpy(R.look_at([0.0, 0.0, 2.0], [0.0, 0.0, 0.0]).astype(np.float32))
    vol.integrate(torch.full_like(depth[0], 5.0), color[0], feat[0], K, back)
    assert not torch.equal(before[2], vol.get_volume()[2])
    vol.reset()
    tsdf, col, wgt, ft = vol.get_volume()
    assert bool((tsdf == 1).all()) and not bool(col.any()) and not bool(wgt.any()) and not bool(ft.any())
    assert tuple(ft.shape) == (*fx["dims"].tolist(), 8) and tuple(col.shape) == (*fx["dims"].tolist(), 3)
    with pytest.raises(ValueError, match="feature images"):
        vol.integrate(depth[0], color[0], feat[0][..., :4], K, poses[0])
    with pytest.raises(ValueError, match="colour images"):
        vol.integrate(depth[0], color[0][:-1], feat[0], K, poses[0])


def _single_frame_check(p, got, depth, color_im, feat_im, K, w2c, trunc, windows=(R.WINDOW_PX, R.WINDOW_M), min_decided=0.98,
                        decided_rows=()):
    """One frame into a fresh volume, at the voxel centres p [S,3]: from w = 0 every operation of the colour and feature means is
    exact ((0 * old + 1 * new) / 1), so weight, colour (rint of the pixel) and the feature row (the pixel's, negatives clamped) must
    equal the restatement exactly on decided voxels.  tsdf = min((d - z) / trunc, 1): z is a sum of three products and a constant,
    six roundings of at most 2^-24 relative to sum |terms| (`zbar`), plus those of the subtraction and the division: the bar is
    (8 * 2^-24 * (zbar + d)) / trunc + 2^-23.  Returns the number of updated voxels among the decided ones."""
    C = feat_im.shape[-1]
    state = R.fresh_state(p.shape[0], C)
    diag = {}
    R.integrate_f64(p, state, depth, color_im, feat_im, K, w2c, 1.0, trunc, diag, windows=windows)
    ok = ~diag["undecided"]
    assert ok.mean() > min_decided and ok[list(decided_rows)].all()
    tsdf, weight, color, feat = got
    assert np.array_equal(weight[ok].astype(np.float64), state["weight"][ok])
    assert np.array_equal(color[ok].astype(np.float64), state["color"][ok])
    assert np.array_equal(feat[ok].astype(np.float64), state["feat"][ok])
    bar = 8 * 2.0 ** -24 * (diag["zbar"] + float(np.max(depth))) / np.float64(np.float32(trunc)) + 2.0 ** -23
    err = np.abs(tsdf.astype(np.float64) - state["tsdf"])
    assert (err[ok] <= bar[ok]).all(), (err[ok].max(), bar[ok].min())
    return int((diag["valid"] & ok).sum())


@pytest.mark.parametrize("feat_dim", [4, 64, 256])
def test_feature_widths(feat_dim):
    vol, fx = _volume("c8", feat_dim=feat_dim)
    depth, color, feat, K, poses = _frames("c8", fx, feat_dim)
    vol.integrate(depth[1], color[1], feat[1], K, poses[1])
    N = int(np.prod(fx["dims"]))
    tsdf, col, wgt, ft = (t.cpu().numpy() for t in vol.get_volume())
    p = R.centres([fx["axis_x"], fx["axis_y"], fx["axis_z"]])
    n = _single_frame_check(p, (tsdf.reshape(N), wgt.reshape(N), col.reshape(N, 3), ft.reshape(N, feat_dim)), fx["depth"][1],
                            color[1].cpu().numpy(), feat[1].cpu().numpy(), fx["K"], fx["w2c"][1], vol.sdf_trunc)
    assert n > 1000
    # the following frames: a batch against singles at this width too
    vol.integrate_frames(depth[2:], color[2:], feat[2:], K, poses[2:])
    batch = _clone(vol)
    vol.reset()
    for f in range(1, R.FRAMES):
        vol.integrate(depth[f], color[f], feat[f], K, poses[f])
    assert _same(batch, vol.get_volume())


def _check_surface(vol, level):
    s = vol.surface(level)
    tsdf, col, _, ft = (t.cpu().numpy() for t in vol.get_volume())
    ref = R.surface_numpy(tsdf, col, ft, level=level, voxel_size=vol.voxel_size, origin=vol.origin.numpy())
    assert float(s["level"]) == float(ref["level"])
    M = ref["verts"].shape[0]
    assert tuple(s["verts"].shape) == (M, 3) and tuple(s["feats"].shape) == (M, vol.feat_dim)
    verts = s["verts"].cpu().numpy()
    # order exact (the comparison is element by element); positions: one f32 division and one addition, the same operations as
    # numpy's: within one ulp of the coordinate
    assert (np.abs(verts - ref["verts"]) <= np.spacing(np.abs(ref["verts"]))).all()
    print(f"\nsurface: {M} vertices at level {float(ref['level'])}; positions bit-equal to numpy: {np.array_equal(verts, ref['verts'])}")
    assert np.array_equal(s["index"].cpu().numpy(), ref["index"])
    assert np.array_equal(s["colors"].cpu().numpy(), ref["colors"])
    assert np.array_equal(s["feats"].cpu().numpy(), ref["feats"])
    pts = (verts * np.float32(vol.voxel_size)).astype(np.float64) + vol.origin.numpy()
    assert np.array_equal(s["points"].cpu().numpy(), pts)
    again = vol.surface(level)
    for k in ("verts", "points", "index", "colors", "feats", "level"):
        assert torch.equal(s[k], again[k]), k
    return M


def test_surface_equals_the_numpy_rule_on_the_device_volume():
    vol, fx = _fused("c256")
    m = _check_surface(vol, None)
    assert abs(m - int(fx["crossing_edges"])) < 0.02 * m       # the reference's volume has about as many crossing edges
    assert _check_surface(vol, 0.0) > 1000
    assert _check_surface(vol, 2.0) == 0                       # a level above every value: an empty cloud, not an error
    pts, cols, feats = vol.feature_cloud()
    assert pts.dtype == torch.float64 and cols.dtype == torch.uint8 and feats.dtype == torch.float32 and pts.is_cuda
    assert pts.shape[0] == cols.shape[0] == feats.shape[0] == m
    lo = vol.origin.numpy()
    hi = lo + (np.array(vol.voxel_dim) - 1) * vol.voxel_size
    assert (pts.cpu().numpy() >= lo - 1e-9).all() and (pts.cpu().numpy() <= hi + 1e-9).all()


def test_surface_of_an_analytic_sphere():
    from splatloc_amd.fusion import TSDFVolume
    dims, centre, radius = (24, 20, 22), (11.3, 9.6, 10.2), 7.25
    vol = TSDFVolume(torch.tensor(dims, dtype=torch.float64), torch.tensor([-1.0, 0.5, 2.0], dtype=torch.float64), 0.02, 4)
    state = {k: v.cpu() for k, v in vol.state().items()}
    state["tsdf"] = torch.from_numpy(R.sphere_sdf(dims, centre, radius))
    state["color"] = torch.from_numpy(np.random.default_rng(0).random((*dims, 3), dtype=np.float32) * 255)
    state["feat"] = torch.from_numpy(np.random.default_rng(1).random((*dims, 4), dtype=np.float32))
    vol.load_state(state)
    m = _check_surface(vol, 0.0)
    s = vol.surface(0.0)
    d = np.sqrt(((s["verts"].cpu().numpy().astype(np.float64) - np.array(centre)) ** 2).sum(axis=1)) - radius
    assert m > 500 and np.abs(d).max() < 0.05
    _check_surface(vol, None)


def test_state_round_trips(tmp_path):
    vol, fx = _fused("c8")
    assert sorted(vol.state()) == ["color", "feat", "tsdf", "weight"]
    torch.save({k: v.cpu() for k, v in vol.state().items()}, tmp_path / "volume.pt")      # the reference's save()
    other, _ = _volume("c8")
    other.load_state(torch.load(tmp_path / "volume.pt"))
    assert _same(vol.get_volume(), other.get_volume())
    a, b = vol.feature_cloud(), other.feature_cloud()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="shape"):
        other.load_state({**vol.state(), "feat": vol.state()["feat"][..., :4]})
    with pytest.raises(ValueError, match="missing"):
        other.load_state({"tsdf": vol.state()["tsdf"]})
    # the two files the decoder's dataset reads
    from splatloc_amd.ply import read_vertex_table
    n = vol.save_feature_cloud(tmp_path / "train" / "mesh.ply", tmp_path / "train" / "feat_cloud.npy")
    table = read_vertex_table(str(tmp_path / "train" / "mesh.ply"))
    assert n == a[0].shape[0] == table["x"].shape[0]
    assert np.array_equal(np.stack([table["x"], table["y"], table["z"]], axis=1), a[0].cpu().numpy().astype(np.float32))
    assert np.array_equal(table["red"], a[1][:, 0].cpu().numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "train" / "feat_cloud.npy"), a[2].cpu().numpy())


def test_decoder_trains_on_the_fused_cloud():
    from tests import decoder_reference as DR
    from splatloc_amd.decoder import FeatureDecoder, train_decoder
    vol, _ = _fused("c256")
    points, _, feats = vol.feature_cloud()
    assert points.shape[0] > 5000 and feats.shape[1] == 256
    torch.manual_seed(0)
    dec = FeatureDecoder(DR.office_0_config()).cuda()
    losses = train_decoder(dec, points, feats, num_epochs=3, batch_size=256)
    steps = -(-points.shape[0] // 256)
    assert losses.shape[0] == 3 * steps and bool(torch.isfinite(losses).all())
    first, last = float(losses[:steps].mean()), float(losses[-steps:].mean())
    print(f"\ncosine loss: first epoch {first:.4f}, third epoch {last:.4f}")
    assert last < first and float(losses[-1]) < float(losses[0])


def test_office_0_sized_volume():
    """300 x 325 x 225 voxels x 256 channels (22.9 GB): one 640 x 480 frame, then sampled voxels, the first and the last voxel of
    the volume included, against the per-voxel restatement.  Skips only when the device has less than 1.5 x the volume free."""
    from splatloc_amd import fusion as F
    bounds = [[-3, 3], [-4, 2.5], [-2, 2.5]]
    voxel_dim, origin = F.grid_from_bounds(bounds, 0.02)
    need, _ = F.volume_bytes(voxel_dim, 256)
    free, _ = torch.cuda.mem_get_info()
    if free < 1.5 * need:
        pytest.skip(f"{free} bytes free, the test needs 1.5 x {need}")
    vol = F.volume_from_bounds(bounds, 0.02, 256, margin=2)
    dims = list(vol.voxel_dim)
    N = dims[0] * dims[1] * dims[2]
    assert dims == [300, 325, 225] and N * 256 > 2 ** 32
    h, w = 480, 640
    K = np.array([[320.0, 0, 319.5], [0, 320.0, 239.5], [0, 0, 1]], np.float32)
    # towards the far (+x, +y, +z) corner (a little off the axis, so that the corner's pixel is no half-integer), the walls 7 cm
    # outside the grid: the last voxel is in view and in free space
    c2w = R.look_at([0.5, -0.5, 0.2], [2.9, 2.3, 2.4]).astype(np.float32)
    depth = R.room_depth(bounds, -0.07, c2w[None].astype(np.float64), K, h, w)[0]
    depth[100:140, 200:260] = 0.0
    gen = torch.Generator(device="cuda").manual_seed(3)
    color = torch.rand((h, w, 3), generator=gen, device="cuda") * 255
    feat = torch.rand((h, w, 256), generator=gen, device="cuda") - 0.4
    vol.integrate(torch.from_numpy(depth), color, feat, torch.from_numpy(K), torch.from_numpy(c2w))
    rng = np.random.default_rng(9)
    idx = np.unique(np.concatenate([[0, N - 1, N - 2, N - 225, N - 225 * 325], rng.integers(0, N, 20000),
                                    rng.integers(N - 2_000_000, N, 20000)]))
    tsdf, col, wgt, ft = vol.get_volume()
    sel = torch.from_numpy(idx).cuda()
    got = (tsdf.view(-1)[sel].cpu().numpy(), wgt.view(-1)[sel].cpu().numpy(), col.view(-1, 3)[sel].cpu().numpy(),
           ft.view(-1, 256)[sel].cpu().numpy())
    axes = [t.numpy() for t in F.axis_tables(voxel_dim, origin, 0.02)]
    x, r = idx // (dims[1] * dims[2]), idx % (dims[1] * dims[2])
    p = np.stack([axes[0][x], axes[1][r // dims[2]], axes[2][r % dims[2]]], axis=1)
    w2c = torch.inverse(torch.from_numpy(c2w).float()).float().numpy()
    # windows for 640 pixels and 8 m: 100 x the f32 rounding of those (2^-14 px, 2^-21 m)
    n = _single_frame_check(p, got, depth, color.cpu().numpy(), feat.cpu().numpy(), K, w2c, vol.sdf_trunc, windows=(1e-2, 1e-4),
                            min_decided=0.9, decided_rows=[0, idx.shape[0] - 1])
    last = N - 1
    print(f"\noffice_0 volume: {n} of {idx.shape[0]} sampled voxels updated; last voxel weight {float(wgt.view(-1)[last])}")
    assert n > 2000
    assert float(wgt.view(-1)[last]) == 1.0 and bool((ft.view(-1, 256)[last] > 0).any())     # the last row of the volume was written
    total = float(wgt.sum(dtype=torch.float64))
    assert total == float((wgt == 1).sum()) and 0.02 * N < total < 0.6 * N
