"""Generates tests/golden/loss_edges.npz: the reference's own float32 loss functions on the CPU on every case of tests/loss_reference.py
(all but the oracle-only grid-stride case), values and autograd gradients:

    refine__<case>__lam<lambda>__{terms,grad}   l1_loss, ssim (gaussian_splatting/utils/loss_utils.py:21-22, 42-102) combined as the
                                                colour-refinement loop does (train_gaussians.py:283-285): terms = (l1, ssim, loss)
    eval__<case>__out                           (psnr, ssim, masked mse, mask count) with the clamp and mask of utils/eval_utils.py:45-52,
                                                psnr / mse of gaussian_splatting/utils/image_utils.py:14-21
    mapping__<case>__<exposure>__{loss,g_image,g_depth,g_marker,g_exposure}
                                                get_loss_mapping (utils/utils.py:55-82) + the three lines of get_loss_marker
                                                (train_gaussians.py:38-42, restated: importing train_gaussians pulls GUI modules)
    <stage>__<case>__checksum                   of the case's inputs: they are not stored, the seeded builders reproduce them
                                                (tests/test_host_loss_edges.py proves it)

Usage: python tests/golden/make_golden_loss_edges.py [path of the reference checkout]   (or SPLATLOC_REFERENCE).  The members carry a fixed
timestamp, so the file regenerates byte for byte.  Only this generator and the fixture (data) are committed.
"""
import io
import os
import sys
import types
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SPLATLOC_REFERENCE", mg.REF)
    sys.path.insert(0, ref)
    from tests import loss_reference as R
    for m in ("cv2", "open3d", "tinycudann", "models"):
        mg.stub(m)
    torch.set_num_threads(1)                       # one summation order, whatever the machine
    out = {}
    with mg.CudaToCpu():
        from gaussian_splatting.utils.image_utils import mse, psnr
        from gaussian_splatting.utils.loss_utils import l1_loss, ssim
        from utils.utils import get_loss_mapping

        for name in R.refine_case_names():
            c = R.refine_case(name)
            out[f"refine__{name}__checksum"] = R.checksum(c["image"], c["gt"])
            gt = torch.from_numpy(c["gt"])
            for lam in R.LAMBDAS:
                image = torch.from_numpy(c["image"].copy()).requires_grad_(True)
                l1 = l1_loss(image, gt)
                s = ssim(image, gt)
                loss = (1.0 - lam) * l1 + lam * (1.0 - s)
                loss.backward()
                out[f"refine__{name}__lam{lam}__terms"] = np.array([l1.item(), s.item(), loss.item()], np.float32)
                out[f"refine__{name}__lam{lam}__grad"] = image.grad.numpy().copy()

        for name in R.eval_case_names():
            c = R.eval_case(name)
            out[f"eval__{name}__checksum"] = R.checksum(c["render"], c["gt"])
            with torch.no_grad():
                rendering, gt_image = torch.from_numpy(c["render"]), torch.from_numpy(c["gt"])
                # ---- utils/eval_utils.py:45-52 ----
                image = torch.clamp(rendering, 0.0, 1.0)
                mask = gt_image.cpu() > 0
                psnr_score = psnr((image[mask]).unsqueeze(0), (gt_image[mask]).unsqueeze(0))
                ssim_score = ssim((image).unsqueeze(0), (gt_image).unsqueeze(0))
                mse_score = mse((image[mask]).unsqueeze(0), (gt_image[mask]).unsqueeze(0))
            out[f"eval__{name}__out"] = np.array([psnr_score.item(), ssim_score.item(), mse_score.item(), float(mask.sum())], np.float64)

        cfg = {"Training": {"rgb_boundary_threshold": float(R.THR)}}
        for name in R.mapping_case_names():
            c = R.mapping_case(name)
            out[f"mapping__{name}__checksum"] = R.checksum(*R.mapping_inputs(c))
            for ex_name, ex in R.EXPOSURES.items():
                image, depth, marker = (torch.from_numpy(c[k].copy()).requires_grad_(True) for k in ("image", "depth", "marker"))
                a = torch.tensor([0.0 if ex is None else ex[0]], dtype=torch.float32, requires_grad=True)
                b = torch.tensor([0.0 if ex is None else ex[1]], dtype=torch.float32, requires_grad=True)
                vp = types.SimpleNamespace(original_image=torch.from_numpy(c["gt_image"]), depth=c["gt_depth"].copy(), exposure_a=a,
                                           exposure_b=b)
                pred = torch.sigmoid(marker.view(-1))
                bce = torch.nn.functional.binary_cross_entropy(pred, torch.from_numpy(c["kp"]).view(-1).float(), reduction="mean")
                lm = get_loss_mapping(cfg, image, depth, vp, None, initialization=ex is None)
                (lm + bce).backward()
                pre = f"mapping__{name}__{ex_name}__"
                out[pre + "loss"] = np.array([lm.item(), bce.item()], np.float32)
                out[pre + "g_image"] = image.grad.numpy().copy()
                out[pre + "g_depth"] = depth.grad.numpy().copy()
                out[pre + "g_marker"] = marker.grad.numpy().copy()
                out[pre + "g_exposure"] = np.array([0.0 if a.grad is None else a.grad.item(), 0.0 if b.grad is None else b.grad.item()],
                                                   np.float32)
    path = os.path.join(HERE, "loss_edges.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
