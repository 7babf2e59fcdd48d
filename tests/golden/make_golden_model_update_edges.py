"""Generates tests/golden/model_update_edges.npz with the reference's own code in THIS container, on the CPU: for every densify case
of tests/model_update_reference.py GaussianModel.densify_and_prune (gaussian_model.py:590-675, with its optimizer surgery), for every
append case GaussianModel.extend_from_pcd (gaussian_model.py:222-241), each on a model whose parameters, Adam state and statistics are
the case's.  The split's torch.normal draw is INJECTED as in make_golden_densify.py: `unit[copy, source_row] * std + mean`, the source
rows read from the caller's own selection mask.

Recorded per case: a checksum of the inputs (the builders are seeded; the host test checks that they still produce what was recorded
from), the new row count, the re-sized xyz and scaling (the two groups the split computes), one checksum over the groups and moments
that are copied, and the step counters.  Only this fixture (data) is committed.  The Adam stride cases are not recorded: oracle only.
"""
import io
import os
import sys
import types
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the repository root and the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import model_update_reference as R  # noqa: E402

GROUPS = R.GROUPS
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
        "marker": "_marker", "kp_score": "_kp_score", "scaling": "_scaling", "rotation": "_rotation"}
ARGS = dict(position_lr_init=0.0016, position_lr_final=0.0000016, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
            feature_lr=0.0025, opacity_lr=0.05, marker_lr=0.05, kp_score_lr=0.05, scaling_lr=0.001, rotation_lr=0.001)


def save_deterministic(path, arrays):
    """np.savez_compressed with fixed member timestamps: the fixture regenerates byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def make_model(GaussianModel, params, m, v, step, percent_dense, primitive_reg):
    gm = GaussianModel(0, config={"Training": {"primitive_reg": primitive_reg}})
    for k in GROUPS:
        setattr(gm, ATTR[k], torch.nn.Parameter(torch.from_numpy(params[k].copy()).requires_grad_(True)))
    gm.max_radii2D = torch.zeros(params["xyz"].shape[0])
    gm.spatial_lr_scale = 6.0
    gm.training_setup(types.SimpleNamespace(percent_dense=percent_dense, **ARGS))
    if m is not None:
        for grp in gm.optimizer.param_groups:
            k = grp["name"]
            if k in m:
                gm.optimizer.state[grp["params"][0]] = {"step": torch.tensor(float(step)), "exp_avg": torch.from_numpy(m[k].copy()),
                                                        "exp_avg_sq": torch.from_numpy(v[k].copy())}
    return gm


def read_model(gm):
    p = {k: getattr(gm, ATTR[k]).detach().numpy().copy() for k in GROUPS}
    m, v, steps = {}, {}, []
    for grp in gm.optimizer.param_groups:
        assert grp["params"][0] is getattr(gm, ATTR[grp["name"]])
        st = gm.optimizer.state.get(grp["params"][0], None)
        if st is not None and len(st):
            m[grp["name"]], v[grp["name"]] = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
            steps.append(float(st["step"]))
    return p, (m or None), (v or None), np.array(steps, np.float64)


def main():
    for mod in ("cv2", "open3d", "tinycudann", "models"):
        mg.stub(mod)
    mg.stub("plyfile", PlyData=object, PlyElement=object)
    mg.stub("models.decoders", FeatureDecoder=object)
    out = {}
    with mg.CudaToCpu():
        from gaussian_splatting.scene.gaussian_model import GaussianModel
        import gaussian_splatting.scene.gaussian_model as gmod
        for name in R.densify_case_names():
            c = R.densify_case(name)
            h = c["hyper"]
            P = c["accum"].shape[0]
            gm = make_model(GaussianModel, c["params"], c["m"], c["v"], c["step"], h["percent_dense"], h["primitive_reg"])
            gm.xyz_gradient_accum, gm.denom = torch.from_numpy(c["accum"].copy()), torch.from_numpy(c["denom"].copy())
            unit = torch.from_numpy(c["unit_noise"].copy())

            def injected_normal(mean, std, **kw):
                mask = sys._getframe(1).f_locals["selected_pts_mask"]        # densify_and_split's own selection
                src = torch.nonzero(mask).reshape(-1)
                assert src.numel() * 2 == std.shape[0] and (src.numel() == 0 or int(src.max()) < P)
                return torch.cat((unit[0, src], unit[1, src]), 0) * std + mean

            real_normal = torch.normal
            torch.normal = gmod.torch.normal = injected_normal
            try:
                gm.densify_and_prune(h["max_grad"], h["min_opacity"], h["extent"], h["max_screen_size"])
            finally:
                torch.normal = gmod.torch.normal = real_normal
            p, m, v, steps = read_model(gm)
            pre = f"densify__{name}__"
            out[pre + "checksum"] = R.checksum(*R.densify_inputs(c))
            out[pre + "rows"] = np.array([p["xyz"].shape[0]], np.float64)
            out[pre + "xyz"], out[pre + "scaling"] = p["xyz"], p["scaling"]
            out[pre + "copied"] = R.outputs_checksum(p, m, v)
            out[pre + "steps"] = steps
            assert not gm.xyz_gradient_accum.any() and not gm.max_radii2D.any()
            print(name, P, "->", p["xyz"].shape[0])
        for name in R.append_case_names():
            c = R.append_case(name)
            gm = make_model(GaussianModel, c["params"], c["m"], c["v"], c["step"], 0.01, False)
            t = lambda a: torch.from_numpy(a.copy())  # noqa: E731
            e = c["extra"]
            gm.extend_from_pcd(t(e["xyz"]), t(c["features"]), t(e["scaling"]), t(e["rotation"]), t(e["opacity"]), t(e["marker"]),
                               t(e["kp_score"]))
            p, m, v, steps = read_model(gm)
            pre = f"append__{name}__"
            out[pre + "checksum"] = R.checksum(*R.append_inputs(c))
            out[pre + "rows"] = np.array([p["xyz"].shape[0]], np.float64)
            out[pre + "all"] = R.checksum(*([p[k] for k in GROUPS] + ([] if m is None else [m[k] for k in GROUPS if k in m]
                                                                   + [v[k] for k in GROUPS if k in v])))
            out[pre + "steps"] = steps
            print(name, "->", p["xyz"].shape[0])
    path = os.path.join(HERE, "model_update_edges.npz")
    save_deterministic(path, out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
