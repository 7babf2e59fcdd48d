"""Generates tests/golden/pnp.npz for solve_pose (test.py:64-84), the conversion of pycolmap's world-to-camera result
(qvec w-first, tvec) into the camera-to-world (R, t) that eval_pose consumes.

solve_pose is extracted from the reference's test.py with ast and run against a stub `pycolmap` module whose
absolute_pose_estimation returns recorded dicts: random unit quaternions, some with w < 0 (the same rotation as -q), a
near-identity and a 180-degree rotation, and one failure ({"success": False}).  Stored per case: the inputs, the recorded dict
and the reference's (R, t), or ref_ok = False for the failure.

Only the fixture (data) is committed; nothing of the reference travels.  Run: python tests/golden/make_golden_pnp.py
<path of the reference checkout> (or set SPLATLOC_REFERENCE).
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_solve_pose(ref, stub):
    src = open(os.path.join(ref, "test.py")).read()
    tree = ast.parse(src)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "solve_pose"]
    assert len(fns) == 1
    from scipy.spatial.transform import Rotation
    ns = {"np": np, "R": Rotation, "pycolmap": stub}
    exec(compile(ast.fix_missing_locations(ast.Module(body=fns, type_ignores=[])), "test.py", "exec"), ns)
    return ns["solve_pose"]


def recorded(rng, k, n):
    if k == 5:
        return {"success": False}
    if k == 3:
        q = np.array([1.0, 1e-9, -2e-9, 3e-9])
    elif k == 4:
        q = np.array([0.0, 0.0, 1.0, 0.0])
    else:
        q = rng.normal(size=4)
    q = q / np.linalg.norm(q)
    if k in (1, 6) and q[0] > 0 or k in (0, 2) and q[0] < 0:
        q = -q
    inl = rng.random(n) < 0.7
    return {"success": True, "qvec": q, "tvec": rng.normal(size=3) * 2.0, "num_inliers": int(inl.sum()), "inliers": inl}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["SPLATLOC_REFERENCE"]
    stub = types.ModuleType("pycolmap")
    solve_pose = reference_solve_pose(ref, stub)
    rng = np.random.default_rng(2026)
    out = {}
    count = 8
    for k in range(count):
        n = 20 + k
        kp2d = rng.uniform(0, 640, size=(n, 2)).astype(np.float32)
        kp3d = rng.normal(size=(n, 3)).astype(np.float32)
        rec = recorded(rng, k, n)
        stub.absolute_pose_estimation = lambda a, b, c, _r=rec: _r
        intr = {"model": "OPENCV", "width": 640, "height": 480, "params": [320.0, 320.0, 319.5, 239.5, 0., 0., 0., 0.]}
        r, t, ret = solve_pose(kp2d, kp3d, intr)
        assert ret is rec
        out.update({f"c{k}_kp2d": kp2d, f"c{k}_kp3d": kp3d, f"c{k}_success": np.bool_(rec["success"]),
                    f"c{k}_ref_ok": np.bool_(r is not None)})
        if rec["success"]:
            out.update({f"c{k}_qvec": rec["qvec"], f"c{k}_tvec": rec["tvec"], f"c{k}_num_inliers": np.int64(rec["num_inliers"]),
                        f"c{k}_inliers": rec["inliers"], f"c{k}_R": np.asarray(r, np.float64), f"c{k}_t": np.asarray(t, np.float64)})
    out["count"] = np.int64(count)
    path = os.path.join(HERE, "pnp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
