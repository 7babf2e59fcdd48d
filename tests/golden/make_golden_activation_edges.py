"""Generates tests/golden/activation_edges.npz: what the reference's OWN code gives on the edge cases of
tests/activation_reference.py, in float64 on the CPU, so that the torch restatement there is pinned to it
(tests/test_host_activation_edges.py).

Per case of CASES (the inputs are rebuilt from the case's seed, only results are stored):
  scales, rotations, opacities   GaussianModel's own activation attributes (gaussian_model.py:57-65: scaling_activation,
                                 rotation_activation, opacity_activation), an isotropic scale repeated as
                                 gaussian_renderer/__init__.py:73-76 does
  colors                         clamp_min(eval_sh(active degree, shs_view, dir) + 0.5, 0) with the reference's eval_sh
                                 (sh_utils.py:55-118) and the view / direction lines of gaussian_renderer/__init__.py:84-90, cat
                                 with the extras (:98-102)
  d_*                            autograd's gradients of sum <output, G> w.r.t. the raw parameters
and two rules of torch itself that the fix and the clamp tests rest on:
  clamp_rule      d clamp_min(x, 0) at x = +0, -0, 1e-30, -1e-30 (float32)
  normalize_sub_eps_*  d normalize at q = (3e-14, 4e-14, 0, 0), g = (1, 2, 3, 4), float32 and float64
Only the fixture (numbers) is committed; the reference never travels.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (sets sys.path for the reference and our stubs)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = ("onehot_deg1", "onehot_deg2", "onehot_deg3", "cw5_p204_deg2", "cw4_p255_deg1of3", "cw3_p256_deg0of3", "clamp0",
         "saturation_deg0", "saturation_deg2")


def main():
    for m in ("cv2", "open3d", "tinycudann", "models"):
        mg.stub(m)
    mg.stub("plyfile", PlyData=object, PlyElement=object)
    mg.stub("models.decoders", FeatureDecoder=object)
    from tests import activation_reference as R
    out = {}
    with mg.CudaToCpu():
        from gaussian_splatting.scene.gaussian_model import GaussianModel
        from gaussian_splatting.utils.sh_utils import eval_sh
        gm = GaussianModel(0, config={"Training": {"primitive_reg": True}})
        for name in CASES:
            c = R.case(name)
            t = {k: torch.from_numpy(np.asarray(c[k], np.float64)).requires_grad_(True) for k in R.INPUTS if c[k] is not None}
            campos = torch.from_numpy(np.asarray(c["campos"], np.float64))
            scales = gm.scaling_activation(t["scaling"])
            if scales.shape[-1] == 1:
                scales = scales.repeat(1, 3)
            rotations = gm.rotation_activation(t["rotation"])
            opacities = gm.opacity_activation(t["opacity"])
            features = torch.cat((t["f_dc"], t["f_rest"]), dim=1)
            shs_view = features.transpose(1, 2).view(-1, 3, c["K"])
            dir_pp = t["xyz"] - campos.repeat(features.shape[0], 1)
            dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
            sh2rgb = eval_sh(c["deg"], shs_view, dir_pp_normalized)
            colors = torch.clamp_min(sh2rgb + 0.5, 0.0)
            if c["E"]:
                colors = torch.cat((colors, t["extra"]), dim=1)
            outs = {"scales": scales, "rotations": rotations, "opacities": opacities, "colors": colors}
            sum((o * torch.from_numpy(np.asarray(c["G_" + k], np.float64))).sum() for k, o in outs.items()).backward()
            for k, o in outs.items():
                out[f"{name}__{k}"] = o.detach().numpy().copy()
            for k in t:
                g = t[k].grad
                out[f"{name}__d_{k}"] = (torch.zeros_like(t[k]) if g is None else g).numpy().copy()
        x = torch.tensor([0.0, -0.0, 1e-30, -1e-30], requires_grad=True)
        torch.clamp_min(x, 0.0).sum().backward()
        out["clamp_rule"] = x.grad.numpy().copy()
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            q = torch.tensor([[3e-14, 4e-14, 0.0, 0.0]], dtype=dt, requires_grad=True)
            (gm.rotation_activation(q) * torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=dt)).sum().backward()
            out["normalize_sub_eps_" + tag] = q.grad.numpy().copy()
    path = os.path.join(HERE, "activation_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    print("clamp_rule", out["clamp_rule"], "normalize_sub_eps_f32", out["normalize_sub_eps_f32"])


if __name__ == "__main__":
    main()
