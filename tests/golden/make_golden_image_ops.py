"""Generates tests/golden/image_ops.npz: the reference's own float32 frame-preparation functions on the CPU on the cases of
tests/image_ops_reference.py:

    mask__<case>__{grad_v,grad_h}   image_gradient (utils/utils.py:4-21) of the gray image, as Camera.compute_grad_mask forms it
    mask__<case>__valid             image_gradient_mask (utils/utils.py:24-38), packed bits (its two masks are asserted equal)
    mask__<case>__out               Camera.compute_grad_mask (utils/camera_utils.py:145-172): float32 [H,W] for "replica", packed bits otherwise
    mask__<case>__{out_bits,err}    the large case instead: the 0 / 1 output as packed bits (it has no remainder and no NaN block) and the
                                    reference's own largest float32 errors of (grad_v, grad_h, intensity) against the float64 oracle, the
                                    oracle's largest intensity
    median__<case>__{out,valid}     get_median_depth(..., return_std=True) (utils/utils.py:85-96): (median, std) float32 and the selection as
                                    packed bits (the reference dereferences `opacity`: cases without one pass ones)
    <stage>__<case>__checksum       of the case's inputs: they are not stored, the seeded builders reproduce them
                                    (tests/test_host_image_ops.py proves it)

Usage: python tests/golden/make_golden_image_ops.py [path of the reference checkout]   (or SPLATLOC_REFERENCE).  The members carry a fixed
timestamp, so the file regenerates byte for byte.  Only this generator and the fixture (data) are committed.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
from make_golden_loss_edges import write_npz  # noqa: E402


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SPLATLOC_REFERENCE", mg.REF)
    sys.path.insert(0, ref)
    from tests import image_ops_reference as R
    for m in ("cv2", "open3d", "tinycudann", "models"):
        mg.stub(m)
    torch.set_num_threads(1)                       # one summation order, whatever the machine
    out = {}
    with mg.CudaToCpu(), torch.no_grad():
        from utils.camera_utils import Camera
        from utils.utils import get_median_depth, image_gradient, image_gradient_mask

        for name in R.GOLDEN_CASES:
            c = R.CASES[name]
            img = R.case_image(name)
            pre = f"mask__{name}__"
            out[pre + "checksum"] = R.checksum(img)
            image = torch.from_numpy(img.copy())
            gray = image.mean(dim=0, keepdim=True)
            gv, gh = image_gradient(gray)
            mv, mh = image_gradient_mask(gray)
            assert torch.equal(mv, mh)
            cam = types.SimpleNamespace(original_image=image, grad_mask=None)
            cfg = {"Training": {"edge_threshold": c["thr"]}, "Dataset": {"type": c["type"]}}
            Camera.compute_grad_mask(cam, cfg)
            res = cam.grad_mask[0].numpy()
            if c["golden"] == "packed":
                assert c["type"] == "replica" and np.isin(res, (0.0, 1.0)).all()
                o = R.grad_mask_model(img, c["thr"], c["type"], np.float64)
                x32 = torch.sqrt((gv * mv) ** 2 + (gh * mh) ** 2)[0].numpy()
                out[pre + "out_bits"] = np.packbits(res != 0)
                out[pre + "err"] = np.array([np.abs(gv[0].numpy() - o["grad_v"]).max(), np.abs(gh[0].numpy() - o["grad_h"]).max(),
                                             np.abs(x32 - o["intensity"]).max(), o["intensity"].max()], np.float64)
                continue
            out[pre + "grad_v"] = gv[0].numpy().copy()
            out[pre + "grad_h"] = gh[0].numpy().copy()
            out[pre + "valid"] = np.packbits(mv[0].numpy())
            out[pre + "out"] = res.astype(np.float32) if c["type"] == "replica" else np.packbits(res)

        for name in R.MEDIAN_GOLDEN:
            c = R.median_case(name)
            pre = f"median__{name}__"
            out[pre + "checksum"] = R.checksum(*[v for v in (c["depth"], c["opacity"], c["mask"]) if v is not None])
            depth = torch.from_numpy(c["depth"].copy())
            opacity = torch.ones_like(depth) if c["opacity"] is None else torch.from_numpy(c["opacity"].copy())
            mask = None if c["mask"] is None else torch.from_numpy(c["mask"].copy())
            med, std, valid = get_median_depth(depth, opacity, mask, return_std=True)
            out[pre + "out"] = np.array([med.item(), std.item()], np.float32)
            out[pre + "valid"] = np.packbits(valid.numpy())
    path = os.path.join(HERE, "image_ops.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
