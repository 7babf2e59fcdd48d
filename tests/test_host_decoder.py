"""Host side of the fused FeatureDecoder: state_dict keys and shapes, configuration errors raised before any device access, the
C ABI's layout validation and workspace sizes, and an import that opens no device.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from tests import decoder_reference as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _config(**decoder):
    cfg = R.office_0_config()
    cfg["decoder"].update(decoder)
    return cfg


def test_state_dict_keys_and_shapes_are_the_reference_ones():
    import torch
    from splatloc_amd.decoder import FeatureDecoder
    fx = R.fixture()                  # written by the reference's own FeatureDecoder on its office_0 yaml
    assert R.fixture_config(fx) == R.office_0_config()
    torch.manual_seed(0)
    dec = FeatureDecoder(R.fixture_config(fx))
    sd = dec.state_dict()
    assert list(sd) == [str(k) for k in fx["state_keys"]]
    assert [list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()] == fx["state_shapes"].tolist()
    assert dec.resolution_sdf == int(fx["resolution_sdf"]) == 108 and dec.embed_dim == 32
    for i, w in enumerate(dec.feature_net.weights()):
        assert torch.equal(w.detach().cpu(), torch.from_numpy(fx[f"w0_{i}"]))
    # the optimiser groups DecoderTrainer hard-wires are the reference's: [lr, beta1, beta2, eps, weight_decay] per group
    from splatloc_amd import decoder as D
    assert fx["optimizer_groups"].tolist() == [[1e-3, D.BETAS[0], D.BETAS[1], D.EPS_WEIGHTS, D.WEIGHT_DECAY],
                                               [1e-3, D.BETAS[0], D.BETAS[1], D.EPS_TABLE, 0.0]]
    # the MLP is initialised as nn.Linear initialises it under the caller's seed; the table consumes none of that stream
    torch.manual_seed(0)
    lin = torch.nn.Linear(32, 128, bias=False)
    assert torch.equal(lin.weight, dec.feature_net.model[0].weight.cpu())
    # the table as splatloc_amd.grid_encoding.Encoding(seed=1337) initialises its own
    init = torch.rand((5_724_048,), generator=torch.Generator().manual_seed(1337), dtype=torch.float32).mul_(2e-4).sub_(1e-4)
    assert torch.equal(init, dec.encoding.params.detach().cpu())


@pytest.mark.parametrize("cfg", [
    _config(hidden_dim=100), _config(hidden_dim=256), _config(hidden_dim=16),
    _config(final_dim=100), _config(final_dim=16), _config(final_dim=288), _config(final_dim=0),
    _config(num_layers=1), _config(num_layers=9),
    _config(enc="freq"), _config(enc="identity"), _config(enc="spherical"), _config(enc="blob"),
    dict(_config(), scene={"bound": [[-1.0, 1.0], [-1.0, 1.0]], "voxel_sdf": 0.06}),
    dict(_config(), scene={"bound": [[-1.0, 1.0, 0.0]] * 3, "voxel_sdf": 0.06}),
    _config(enc="dense"),            # 4 levels x 2 features: an encoded width of 8 is not a multiple of 16
])
def test_unsupported_configurations_raise_before_any_device_access(cfg):
    code = ("import torch, sys; from splatloc_amd.decoder import FeatureDecoder\n"
            f"cfg = {cfg!r}\n"
            "try:\n    FeatureDecoder(cfg)\nexcept ValueError as e:\n    assert 'supported' in str(e), e\nelse:\n    sys.exit('no error')\n"
            "assert not torch.cuda.is_initialized(); print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-2000:])


def test_fixture_batches_have_no_undecided_point():
    """the generator's assertion, run here: every point of the three fixture batches has all its hidden pre-activations outside
    their f32 rounding bar of zero under the initial model, so the share of excluded points is 0 (cap: 1 %).  The pools the
    batches were taken from had `pool_undecided` such points (about 1.8 %: unfiltered uniform batches would not meet the cap)."""
    import torch
    from splatloc_amd.decoder import FeatureDecoder
    fx = R.fixture()
    torch.manual_seed(0)
    ref = R.RestatedDecoder(FeatureDecoder(R.fixture_config(fx)))
    for k in range(3):
        assert bool(ref.decided(torch.from_numpy(fx["batches"][k])).all()), k
    assert 0 < int(fx["pool_undecided"][0]) <= 0.03 * int(fx["pool_undecided"][1])


def test_input_ch_other_than_3_raises():
    from splatloc_amd.decoder import FeatureDecoder
    with pytest.raises(ValueError, match="supported"):
        FeatureDecoder(R.office_0_config(), input_ch=2)


def _layout(dims, levels=16, features=2):
    from splatloc_amd import _native
    from splatloc_amd.grid_encoding import GridLayout
    lay = _native.DecoderLayout()
    lay.grid = GridLayout(3, {"otype": "HashGrid", "n_levels": levels, "n_features_per_level": features, "per_level_scale": 1.3}).native
    for k, (lo, hi) in enumerate(R.OFFICE_0):
        lay.bound[k][0], lay.bound[k][1] = lo, hi
    lay.n_layers = len(dims) - 1
    for i, v in enumerate(dims[:9]):
        lay.dims[i] = v
    return lay


def test_workspace_bytes_and_layout_validation_run_on_the_host():
    from splatloc_amd import _native
    lib = _native.load()
    ws, act = C.c_size_t(0), C.c_size_t(0)
    lay = _layout([32, 128, 128, 128, 256])
    assert lib.splatraster_decoder_workspace_bytes(C.byref(lay), 256, C.byref(ws), C.byref(act)) == 0
    # activations: encoded + three hidden + f + norm + normalised points; workspace: 8 slabs of 69 632 floats + 8 loss terms + dL/denc
    assert act.value == 4 * 256 * (32 + 3 * 128 + 256 + 1 + 3)
    assert ws.value == 8 * 69_632 * 4 + 256 + 256 * 32 * 4
    assert lib.splatraster_decoder_workspace_bytes(C.byref(lay), 1_000_000, C.byref(ws), None) == 0
    assert ws.value == 64 * 69_632 * 4 + 31_250 * 4 + 184 + 1_000_000 * 32 * 4       # the workgroups of the backward are bounded
    assert lib.splatraster_decoder_workspace_bytes(C.byref(lay), 0, C.byref(ws), C.byref(act)) == 0 and act.value == 0
    assert lib.splatraster_decoder_workspace_bytes(None, 256, C.byref(ws), C.byref(act)) == 1
    assert lib.splatraster_decoder_workspace_bytes(C.byref(lay), -1, C.byref(ws), C.byref(act)) == 1
    for dims, levels, features in [([32, 128, 64, 256], 16, 2),      # two hidden widths
                                   ([32, 96, 256], 16, 2), ([32, 128, 48], 16, 2), ([32, 128, 512], 16, 2), ([32, 256], 16, 2),
                                   ([32] + [64] * 8 + [32], 16, 2),  # nine layers
                                   ([64, 128, 256], 16, 2),          # dims[0] is not L*F
                                   ([24, 64, 32], 12, 2), ([128, 64, 32], 16, 8)]:
        assert lib.splatraster_decoder_workspace_bytes(C.byref(_layout(dims, levels, features)), 256, C.byref(ws), C.byref(act)) == 1, dims
    for dims, levels, features in [([16, 32, 32], 8, 2), ([48, 64, 64, 96], 12, 4), ([64, 128] + [128] * 6 + [256], 16, 4)]:
        assert lib.splatraster_decoder_workspace_bytes(C.byref(_layout(dims, levels, features)), 256, C.byref(ws), C.byref(act)) == 0, dims
    # every entry point validates before it launches: null pointers with a valid layout are bad arguments, not faults
    assert lib.splatraster_decoder_forward(C.byref(lay), 4, None, 0, None, None, None, None, None) == 1
    assert lib.splatraster_decoder_backward(C.byref(lay), 4, None, None, None, None, None, None, None, None, None, None, None) == 1
    bad = _layout([32, 128, 128, 128, 256])
    bad.grid.offset[3] += 8
    assert lib.splatraster_decoder_workspace_bytes(C.byref(bad), 4, C.byref(ws), C.byref(act)) == 1


def test_import_opens_no_device():
    code = ("import torch, splatloc_amd.decoder; from splatloc_amd.decoder import FeatureDecoder, DecoderTrainer, train_decoder, "
            "cos_loss, l2_loss; assert not torch.cuda.is_initialized(); print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
