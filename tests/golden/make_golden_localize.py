"""Generates tests/golden/localize.npz for the localisation stage (splatloc_amd/localize.py):

    generate_retrieval_file   pre_process/gen_netvlad_retrieval.py:15-42   imported from the reference with stub `hloc` modules
                                                                           in sys.modules that hand it the generator's arrays
    eval_pose, SO3_to_quat,   utils/eval_utils.py:75-145                   extracted with ast (eval_utils imports cv2)
    compute_quaternion_dist

Retrieval cases (r<c>_*): rebuilt from seeds by tests/localize_reference.py (elementwise numpy, bit-identical everywhere), so
only the seed, the shape, a sha256 of the arrays and the reference's results are stored: `ind` (parsed back from the file the
reference wrote) and `sims` (its formula, torch.einsum("id,jd->ij").topk, on the same f32 arrays).  Case 1 also stores the file.
The generator asserts that the reference's f32 indices equal the f64 restatement's.

Pose cases (p_*): 400 poses, R_est = dR(angle) R_gt about a random axis, angles {0, 1e-6, 1e-4, 1e-3, 0.01, 0.05} degrees,
log-uniform angles in [0.1, 178] degrees and a half turn about z; every SO3_to_quat branch occurs.  f64 inputs and the
reference's thetas / dists are stored.

Only the fixture (data) is committed; nothing of the reference travels.  Run: python tests/golden/make_golden_localize.py
<path of the reference checkout> (or set SPLATLOC_REFERENCE).
"""
import ast
import math
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import localize_reference as LR  # noqa: E402


def reference_generate(ref):
    """the reference's generate_retrieval_file, fed from a registry {path: (names, descriptors)}"""
    import torch
    registry = {}
    hloc = types.ModuleType("hloc")
    ef = types.ModuleType("hloc.extract_features")
    pr = types.ModuleType("hloc.pairs_from_retrieval")
    ut = types.ModuleType("hloc.utils")
    io = types.ModuleType("hloc.utils.io")
    io.list_h5_names = lambda path: list(registry[path][0])
    pr.parse_names = lambda prefix, names, names_all: list(names_all)

    def get_descriptors(names, path, name2idx=None):
        paths = path if isinstance(path, list) else [path]
        rows = []
        for n in names:
            src = paths[name2idx[n]] if name2idx is not None else paths[0]
            rows.append(registry[src][1][registry[src][0].index(n)])
        return torch.from_numpy(np.stack(rows)).float()

    pr.get_descriptors = get_descriptors
    hloc.extract_features, hloc.pairs_from_retrieval, hloc.utils, ut.io = ef, pr, ut, io
    for name, mod in (("hloc", hloc), ("hloc.extract_features", ef), ("hloc.pairs_from_retrieval", pr), ("hloc.utils", ut),
                      ("hloc.utils.io", io)):
        sys.modules[name] = mod
    sys.path.insert(0, os.path.join(ref, "pre_process"))
    import gen_netvlad_retrieval as g
    return g.generate_retrieval_file, registry


def retrieval_cases(ref):
    import torch
    generate, registry = reference_generate(ref)
    out = {}
    for case, (seed, Q, N, D, k) in LR.RETRIEVAL_CASES.items():
        q, db, _, draws = LR.retrieval_case(case)
        qn = [f"query_{i:04d}.jpg" for i in range(Q)]
        dn = [f"frame_{i:05d}.jpg" for i in range(N)]
        registry["q"], registry["d"] = (qn, q), (dn, db)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "netvlad_retrieval.txt")
            generate("q", "d", path, num_matched=k)
            text = open(path).read()
        lut = {n: i for i, n in enumerate(dn)}
        lines = text.split("\n")[:-1]
        assert [ln.split(" ")[0] for ln in lines] == qn
        ind = np.array([[lut[n] for n in ln.split(" ")[1:]] for ln in lines], np.int64)
        sims, ind1 = torch.einsum("id,jd->ij", torch.from_numpy(q), torch.from_numpy(db)).topk(k, dim=1, largest=True)
        assert np.array_equal(ind1.numpy(), ind)
        idx64, s64 = LR.retrieval_topk(q, db, k)
        assert np.array_equal(idx64, ind), f"case {case}: the reference's f32 indices differ from f64"
        err = float(np.abs(sims.numpy().astype(np.float64) - s64).max())
        print(f"case {case}: Q={Q} N={N} D={D} k={k}: {draws} draws, |sims - f64| <= {err:.2e}")
        out.update({f"r{case}_shape": np.array([seed, Q, N, D, k], np.int64), f"r{case}_ind": ind, f"r{case}_sims": sims.numpy(),
                    f"r{case}_sha256": np.array(LR.case_hash(q, db))})
        if case == 1:
            out["r1_text"] = np.array(text)
    return out


def reference_eval_pose(ref):
    import torch
    import torch.nn.functional as F
    tree = ast.parse(open(os.path.join(ref, "utils", "eval_utils.py")).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("compute_quaternion_dist", "SO3_to_quat", "eval_pose")]
    assert len(fns) == 3
    ns = {"torch": torch, "F": F, "math": math, "np": np}
    exec(compile(ast.fix_missing_locations(ast.Module(body=fns, type_ignores=[])), "eval_utils.py", "exec"), ns)
    return ns["eval_pose"]


def rodrigues(axis, deg):
    a = math.radians(deg)
    x, y, z = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * (Kx @ Kx)


def random_rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def pose_cases(ref):
    import torch
    eval_pose = reference_eval_pose(ref)
    rng = np.random.default_rng(31)
    B = 400
    small = [0.0, 1e-6, 1e-4, 1e-3, 0.01, 0.05]
    angles = np.array(small * 4 + list(np.exp(rng.uniform(math.log(0.1), math.log(178.0), size=B - 4 * len(small) - 1))) + [180.0])
    R_gt = np.stack([random_rotation(rng) for _ in range(B)])
    R_est = np.stack([rodrigues(rng.standard_normal(3), a) @ R_gt[b] for b, a in enumerate(angles[:-1])]
                     + [rodrigues(np.array([0.0, 0.0, 1.0]), 180.0) @ R_gt[-1]])
    t_gt = rng.uniform(-5, 5, size=(B, 3))
    t_est = t_gt + rng.standard_normal((B, 3)) * np.exp(rng.uniform(math.log(1e-4), math.log(1.0), size=(B, 1)))
    for R in (R_gt, R_est):
        assert {LR.quat_branch(r) for r in R} == {1, 2, 3, 4}
    thetas, dists = eval_pose(torch.from_numpy(R_est), torch.from_numpy(t_est), torch.from_numpy(R_gt), torch.from_numpy(t_gt))
    thetas, dists = thetas.numpy(), dists.numpy()
    assert thetas.shape == (B, 1, 1) and thetas.dtype == np.float32 and dists.shape == (B,) and dists.dtype == np.float64
    th = thetas.reshape(-1)
    floor = th[:4 * len(small)]
    assert np.all(floor == floor[0]) and abs(float(floor[0]) - 0.05595291) < 1e-7, floor
    assert abs(float(th[-1]) - 180.0) < 1e-3
    big = angles[4 * len(small):]
    print("pose: floor %.8f, |theta - planted| / bound <= %.2f" %
          (float(floor[0]), float((np.abs(th[4 * len(small):] - big) / LR.theta_bound(big)).max())))
    return {"p_angles": angles, "p_R_est": R_est, "p_t_est": t_est, "p_R_gt": R_gt, "p_t_gt": t_gt, "p_thetas": thetas,
            "p_dists": dists}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["SPLATLOC_REFERENCE"]
    out = {}
    out.update(retrieval_cases(ref))
    out.update(pose_cases(ref))
    path = os.path.join(HERE, "localize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
