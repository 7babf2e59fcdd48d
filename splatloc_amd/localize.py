"""Localisation of SplatLoc's test.py --eval_pose from global descriptors to median errors, on the device.

`retrieve` is pre_process/gen_netvlad_retrieval.py's einsum + topk as one fused kernel (csrc/retrieval.hip: the Q x N similarity
matrix never exists), `write_retrieval_file` / `load_retrieval_results` / `generate_retrieval_file` keep the reference's text
format, `pose_errors` / `eval_pose` are utils/eval_utils.py:75-145, and `Localizer` joins the per-query stages (frustum
candidates, FeatureDecoder, Hungarian matching, P3P LO-RANSAC) for a batch of queries.  There is no CPU
fallback: without the device the calls raise.  Argument checks that need no data run before any device work.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native, matching, pnp
from ._host import _stream, device, float_tensor, ptr, workspace

MAX_K = 128                 # SPLATRASTER_RETRIEVAL_MAX_K
RETRIEVAL_OK, RETRIEVAL_NONFINITE = 0, 1
MIN_CANDIDATES = 5          # test.py:318: fewer candidates of the retrieved frame fail the query
MIN_MATCHES = 4             # pnp's rule: fewer correspondences give no model
Z_FLOOR = -10000.0          # test.py:344 kp_3d_mask
_FLOATS = (torch.float16, torch.float32, torch.float64)


def _descriptors(a, what):
    """numpy / torch f16, f32 or f64 [rows, D] (checked, not yet moved or converted)"""
    # converted first, so that a refused numpy array is named by its torch dtype like any other input
    t = float_tensor(torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a, what, _FLOATS)
    if t.dim() != 2:
        raise ValueError(f"{what} must be [rows, D], got {tuple(t.shape)}")
    return t


def retrieve(query_desc, db_desc, k=10):
    """The k most similar database rows of every query row: (idx int64 [Q, k], sims f32 [Q, k]) device tensors, similarity
    descending, equal similarities by database index ascending.  query_desc [Q, D], db_desc [N, D]: numpy or torch, f16 / f32 /
    f64 (converted to f32).  ValueError for a wrong rank, differing D, k outside [1, min(N, 128)], and for descriptors that give
    a NaN similarity ("descriptors contain non-finite entries").  One host read (the status)."""
    q, d = _descriptors(query_desc, "query descriptors"), _descriptors(db_desc, "database descriptors")
    Q, D, N = int(q.shape[0]), int(q.shape[1]), int(d.shape[0])
    if int(d.shape[1]) != D:
        raise ValueError(f"descriptor dimensions differ: {D} and {int(d.shape[1])}")
    if D < 1 or N < 1:
        raise ValueError(f"retrieval needs at least one database row and one dimension, got N = {N}, D = {D}")
    if N >= 1 << 31:
        raise ValueError(f"{N} database rows: fewer than 2^31 are supported")
    k = int(k)
    if not 1 <= k <= min(N, MAX_K):
        raise ValueError(f"k = {k} must lie in [1, min(N, {MAX_K})] (N = {N})")
    dev = device("localisation")
    q = q.detach().to(device=dev, dtype=torch.float32).contiguous()
    d = d.detach().to(device=dev, dtype=torch.float32).contiguous()
    idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
    sims = torch.empty((Q, k), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    lib = _native.load()
    ws = workspace(lib.splatraster_retrieval_workspace_bytes(Q, N, D, k), dev)
    _native.check(lib.splatraster_retrieval_topk(Q, N, D, k, ptr(q), ptr(d), ptr(idx), ptr(sims), ptr(status), ptr(ws),
                                                 _stream(dev)), "splatraster_retrieval_topk")
    if int(status.cpu()[0]) != RETRIEVAL_OK:   # the one host read of the call
        raise ValueError("descriptors contain non-finite entries")
    return idx, sims


def write_retrieval_file(path, query_names, db_names, idx):
    """netvlad_retrieval.txt as gen_netvlad_retrieval.py:36-42 writes it: per query `name db_1 ... db_k\\n`"""
    ind = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx)
    if ind.ndim != 2 or ind.shape[0] != len(query_names):
        raise ValueError(f"idx must be [{len(query_names)}, k], got {ind.shape}")
    if ind.size and (ind.min() < 0 or ind.max() >= len(db_names)):
        raise ValueError(f"idx refers to database rows outside [0, {len(db_names)})")
    with open(path, "w") as f:
        for i in range(ind.shape[0]):
            f.write(query_names[i])
            for j in range(ind.shape[1]):
                f.write(" ")
                f.write(db_names[int(ind[i, j])])
            f.write("\n")


def load_retrieval_results(path):
    """{query name: [database names, best first]} with LocalizeQuery.load_retrieval_results' parsing (test.py:167-177)"""
    results = {}
    with open(path, "r") as f:
        lines = f.readlines()
    for line in lines:
        names = line.replace("\n", "").split(" ")
        results[names[0]] = names[1:]
    return results


def generate_retrieval_file(query_desc, db_desc, query_names, db_names, out_path, num_matched=10):
    """gen_netvlad_retrieval.py's generate_retrieval_file on arrays: query_desc [Q, D] / db_desc [N, D] are the global
    descriptors in the order of query_names / db_names.  Returns (idx, sims) of `retrieve`."""
    nq = int(query_desc.shape[0]) if hasattr(query_desc, "shape") else len(query_desc)
    nd = int(db_desc.shape[0]) if hasattr(db_desc, "shape") else len(db_desc)
    if nq != len(query_names) or nd != len(db_names):
        raise ValueError(f"{nq} query / {nd} database descriptors for {len(query_names)} / {len(db_names)} names")
    idx, sims = retrieve(query_desc, db_desc, k=num_matched)
    write_retrieval_file(out_path, query_names, db_names, idx)
    return idx, sims


def _poses(R, t, what):
    """checked (R [B, 3, 3], t [B, 3]) float tensors (not yet moved or widened)"""
    R = torch.from_numpy(np.ascontiguousarray(R)) if isinstance(R, np.ndarray) else torch.as_tensor(R)
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else torch.as_tensor(t)
    if R.dtype not in _FLOATS or t.dtype not in _FLOATS:
        raise ValueError(f"{what} poses must be floating point, got {R.dtype} and {t.dtype}")
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] != R.shape[0]:
        raise ValueError(f"{what} poses must be R [B, 3, 3] and t [B, 3], got {tuple(R.shape)} and {tuple(t.shape)}")
    return R, t


def pose_errors(R_est, t_est, R_gt, t_gt, valid=None):
    """eval_pose's two numbers per pose: device (theta_deg f32 [B], dist f64 [B]).  Rotations [B, 3, 3] and translations
    [B, 3] (numpy or torch, any float type, widened to f64 exactly); rows with valid == 0 get NaN."""
    Re, te = _poses(R_est, t_est, "estimated")
    Rg, tg = _poses(R_gt, t_gt, "ground-truth")
    B = int(Re.shape[0])
    if int(Rg.shape[0]) != B:
        raise ValueError(f"{B} estimated and {int(Rg.shape[0])} ground-truth poses")
    if valid is not None:
        valid = torch.as_tensor(valid).reshape(-1)
        if valid.shape[0] != B:
            raise ValueError(f"valid must hold {B} values, got {valid.shape[0]}")
    dev = device("localisation")
    f64 = lambda x: x.detach().to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
    Re, te, Rg, tg = f64(Re), f64(te), f64(Rg), f64(tg)
    v = None if valid is None else (valid.to(dev) != 0).to(torch.uint8).contiguous()
    theta = torch.empty(B, dtype=torch.float32, device=dev)
    dist = torch.empty(B, dtype=torch.float64, device=dev)
    _native.check(_native.load().splatraster_pose_errors(B, ptr(Re), ptr(te), ptr(Rg), ptr(tg), ptr(v), ptr(theta),
                                                         ptr(dist), _stream(dev)), "splatraster_pose_errors")
    return theta, dist


def eval_pose(eval_Rs, eval_ts, gt_Rs, gt_ts, show_results=False):
    """Drop-in for utils/eval_utils.py's eval_pose: CPU (thetas f32 [B, 1, 1], dists [B] in eval_ts' float type)."""
    theta, dist = pose_errors(eval_Rs, eval_ts, gt_Rs, gt_ts)
    ts = torch.as_tensor(eval_ts)
    thetas = theta.cpu().reshape(-1, 1, 1)
    dists = dist.cpu().to(torch.result_type(ts, torch.as_tensor(gt_ts)))
    if show_results:
        print("translation_error: ", dists)
        print("rotation_error: ", thetas)
    return thetas, dists


def _median(values, keep):
    """numpy's median of values[keep] on the device (mean of the two middle values for an even count, NaN for none)"""
    if values.numel() == 0:
        return torch.full((), float("nan"), dtype=values.dtype, device=values.device)
    n = keep.sum()
    s = torch.sort(torch.where(keep, values, torch.full_like(values, float("inf")))).values
    lo = torch.clamp(torch.div(n - 1, 2, rounding_mode="floor"), min=0).reshape(1)
    hi = torch.clamp(torch.div(n, 2, rounding_mode="floor"), max=values.numel() - 1).reshape(1)
    m = ((s.gather(0, lo) + s.gather(0, hi)) / 2).reshape(())
    return torch.where(n > 0, m, torch.full_like(m, float("nan")))


class PoseReport:
    """per-query errors and the medians of test.py:498-513 (host values)"""

    def __init__(self, success, retrieval_theta, retrieval_dist, match_theta, match_dist, medians):
        self.success = success                    # bool [Q]
        self.retrieval_theta = retrieval_theta    # f32 [Q] degrees, NaN for failed queries
        self.retrieval_dist = retrieval_dist      # f64 [Q]
        self.match_theta = match_theta
        self.match_dist = match_dist
        (self.median_retrieval_theta, self.median_retrieval_dist, self.median_match_theta,
         self.median_match_dist) = medians        # np.float32, np.float64, np.float32, np.float64

    def format_report(self):
        """the text of eval_pose.txt: the header and the two lines of test.py:510-512"""
        return ("Median Error: \n"
                "Retrieval: Trans.(cm): {}. Rotation(deg): {}.\n".format(self.median_retrieval_dist * 100,
                                                                         self.median_retrieval_theta)
                + "Match    : Trans.(cm): {}. Rotation(deg): {}.\n".format(self.median_match_dist * 100,
                                                                           self.median_match_theta))


class Localizer:
    """LocalizeQuery.match_feature (test.py:304-377) for a batch of queries.

    points / marker: the key Gaussians' xyz and marker; decoder: the FeatureDecoder; K / width / height: the training
    dataset's intrinsics and size (get_frusm_pts); intrinsics: the pycolmap-style camera dict of solve_pose; subset: the
    --eval_selection landmarks (frustum culling only, the points keep their dtype)."""

    def __init__(self, points, marker, decoder, K, width, height, intrinsics, subset=None, max_cost_elements=1 << 27):
        self.points, self.marker, self.decoder, self.K = points, marker, decoder, K
        self.width, self.height = int(width), int(height)
        self.intr = pnp.camera_intrinsics(intrinsics)
        self.subset = subset
        if subset is not None:
            s = torch.as_tensor(subset)
            if s.dtype not in (torch.float32, torch.float64) or s.dim() != 2 or s.shape[1] != 3:
                raise ValueError(f"subset must be float32 or float64 [M, 3], got {s.dtype} {tuple(s.shape)}")
        self._subset_dev = None
        self.max_cost_elements = int(max_cost_elements)   # f64 cost entries held at a time (one LSAP launch per such chunk)

    def _candidates(self, frame, dev):
        """(xyz [n, 3] as the per-query path hands it to solve_pose, descriptors [C, n] f32) of a database frame, or None"""
        if self.subset is not None:
            idx, xyz, _ = matching.frustum_candidates(self.subset, frame["w2c"], self.K, self.width, self.height)
            if self._subset_dev is None:
                self._subset_dev = torch.as_tensor(self.subset).detach().to(dev)
            xyz = self._subset_dev[idx]
        else:
            idx, xyz, _ = matching.frustum_candidates(self.points, frame["w2c"], self.K, self.width, self.height,
                                                      marker=self.marker, kp_mask=frame["sp_kp_mask"], depth=frame["depth"],
                                                      c2w=frame["c2w"], kp_K=frame["K"])
        if xyz.shape[0] < MIN_CANDIDATES:
            return None
        feats = self.decoder(xyz)
        return xyz, feats.detach().to(device=dev, dtype=torch.float32).t().contiguous()

    @torch.no_grad()
    def localize(self, queries, db_frames, db_index):
        """queries: [{"keypoints" [n, 2], "descriptors" [C, n]}]; db_frames: dataset frames (w2c, c2w, K, depth, sp_kp_mask);
        db_index[i]: the top-1 retrieved frame of query i.  Returns device tensors {"R_c2w" [Q,3,3], "t_c2w" [Q,3] (f64),
        "success" bool [Q], "num_inliers" i32 [Q], "retrieval_R", "retrieval_t"}; failed queries carry the retrieval pose, as
        test.py:318-326 returns it.  Host reads: the candidate count of each distinct frame, one per LSAP launch."""
        Q = len(queries)
        index = [int(i) for i in db_index]
        if len(index) != Q:
            raise ValueError(f"{Q} queries and {len(index)} retrieved frames")
        if any(not 0 <= i < len(db_frames) for i in index):
            raise ValueError(f"db_index refers to frames outside [0, {len(db_frames)})")
        kps, descs = [], []
        for qi, q in enumerate(queries):
            kp = float_tensor(q["keypoints"], "keypoints")
            ds = float_tensor(q["descriptors"], "descriptors")
            if kp.dim() != 2 or kp.shape[1] != 2 or ds.dim() != 2 or ds.shape[1] != kp.shape[0]:
                raise ValueError(f"query {qi}: keypoints must be [n, 2] and descriptors [C, n], got {tuple(kp.shape)} and "
                                 f"{tuple(ds.shape)}")
            if not kp.is_cuda and not bool(torch.isfinite(kp).all()):
                raise ValueError(f"query {qi}: keypoints must be finite")
            kps.append(kp)
            descs.append(ds)
        opt = pnp.options(**pnp.DEFAULTS)
        dev = device("localisation")
        lib = _native.load()
        stream = _stream(dev)
        if Q == 0:
            e = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
            return {"R_c2w": e(0, 3, 3), "t_c2w": e(0, 3), "success": e(0, dtype=torch.bool), "num_inliers": e(0, dtype=torch.int32),
                    "retrieval_R": e(0, 3, 3), "retrieval_t": e(0, 3)}
        self._subset_dev = None
        distinct = list(dict.fromkeys(index))
        cand = {f: self._candidates(db_frames[f], dev) for f in distinct}
        c2w = torch.stack([torch.as_tensor(db_frames[f]["c2w"]).detach().to("cpu", torch.float64) for f in distinct]).to(dev)
        slot = {f: s for s, f in enumerate(distinct)}
        which = torch.tensor([slot[f] for f in index], dtype=torch.int64, device=dev)
        retrieval_R = c2w[which, :3, :3].contiguous()
        retrieval_t = c2w[which, :3, 3].contiguous()

        # queries that reach the matcher, in chunks that bound the cost matrices held at once
        run = []
        for qi in range(Q):
            c = cand[index[qi]]
            if c is None:
                continue
            n1, n2 = int(kps[qi].shape[0]), int(c[0].shape[0])
            if descs[qi].shape[0] != c[1].shape[0]:
                raise ValueError(f"descriptor dimensions differ: {descs[qi].shape[0]} and {c[1].shape[0]}")
            if max(n1, n2) > matching.MAX_NC or n1 * n2 >= matching.MAX_ELEMENTS:
                raise ValueError(f"{n1} x {n2} descriptors: the device solver takes at most {matching.MAX_NC} of the larger set "
                                 "and fewer than 2^31 pairs")
            if min(n1, n2) >= MIN_MATCHES:
                run.append(qi)
        chunks, cur, cur_el = [], [], 0
        for qi in run:
            el = int(kps[qi].shape[0]) * int(cand[index[qi]][0].shape[0])
            if cur and cur_el + el > self.max_cost_elements:
                chunks.append(cur)
                cur, cur_el = [], 0
            cur.append(qi)
            cur_el += el
        if cur:
            chunks.append(cur)
        items = []
        for chunk in chunks:
            sizes = [(int(kps[qi].shape[0]), int(cand[index[qi]][0].shape[0])) for qi in chunk]
            cost = torch.empty(sum(a * b for a, b in sizes), dtype=torch.float64, device=dev)
            problems, off, total = [], 0, 0
            for qi, (n1, n2) in zip(chunk, sizes):
                a = descs[qi].detach().to(device=dev, dtype=torch.float32).contiguous()
                b = cand[index[qi]][1]
                norms = torch.empty(n1 + n2, dtype=torch.float32, device=dev)
                matching._cost_launch(a, b, matching.THRESHOLD, norms, cost, off, dev)
                problems.append(matching.LsapProblem(off, min(n1, n2), max(n1, n2), int(n2 < n1), 0))
                off += n1 * n2
                total += min(n1, n2)
            B = len(problems)
            rows, cols, status, _ = matching._lsap_launch(cost, problems, B, False, dev, total)
            # test.py:344 drops matched points with z <= -10000: decided for the chunk's frames at once
            z_ok = torch.stack([(cand[f][0][:, 2] > Z_FLOOR).all() for f in dict.fromkeys(index[qi] for qi in chunk)]).all()
            host = torch.cat([status, z_ok.to(torch.int32).reshape(1)]).cpu()   # the one host read of the chunk
            matching._lsap_raise(host[:B])
            o = 0
            for qi, (n1, n2) in zip(chunk, sizes):
                k = min(n1, n2)
                p2 = kps[qi].detach().to(dev)[rows[o:o + k]]
                p3 = cand[index[qi]][0][cols[o:o + k]]
                o += k
                if not bool(host[B]):   # a host read per query, only for scenes with such points
                    keep = p3[:, 2] > Z_FLOOR
                    p2, p3 = p2[keep], p3[keep]
                items.append((qi, p2, p3))
        items = [it for it in items if it[1].shape[0] >= MIN_MATCHES]

        R = retrieval_R.transpose(1, 2).contiguous()   # placeholders: inverted below, then replaced by the retrieval pose
        t = torch.zeros((Q, 3), dtype=torch.float64, device=dev)
        success = torch.zeros(Q, dtype=torch.bool, device=dev)
        ninl = torch.zeros(Q, dtype=torch.int32, device=dev)
        if items:
            if len(items) > 65535:
                raise ValueError("at most 65535 queries reach the pose stage of one batch")
            solved = pnp._solve([(p2, p3, self.intr) for _, p2, p3 in items], opt, dev)
            sel = torch.tensor([qi for qi, _, _ in items], dtype=torch.int64, device=dev)
            R[sel] = torch.stack([r["R"] for r in solved])
            t[sel] = torch.stack([r["t"] for r in solved])
            success[sel] = torch.stack([r["success"] for r in solved])
            ninl[sel] = torch.stack([r["num_inliers"] for r in solved])
        R_c2w = torch.empty_like(R)
        t_c2w = torch.empty_like(t)
        _native.check(lib.splatraster_pose_invert(Q, ptr(R), ptr(t), ptr(R_c2w), ptr(t_c2w), stream),
                      "splatraster_pose_invert")
        ok = success.reshape(-1, 1)
        return {"R_c2w": torch.where(ok.reshape(-1, 1, 1), R_c2w, retrieval_R), "t_c2w": torch.where(ok, t_c2w, retrieval_t),
                "success": success, "num_inliers": torch.where(success, ninl, torch.zeros_like(ninl)),
                "retrieval_R": retrieval_R, "retrieval_t": retrieval_t}

    def evaluate(self, result, gt_c2w):
        """Errors of the retrieval pose and of the matched pose against gt_c2w [Q, 4, 4] (the queries' camera-to-world), and
        numpy's medians over the successful queries, as test.py:473-513 reports them.  One host read."""
        gt = torch.stack([torch.as_tensor(g) for g in gt_c2w]) if isinstance(gt_c2w, (list, tuple)) else torch.as_tensor(gt_c2w)
        Q = int(result["success"].shape[0])
        if tuple(gt.shape) != (Q, 4, 4) or gt.dtype not in _FLOATS:
            raise ValueError(f"gt_c2w must be a float [{Q}, 4, 4], got {gt.dtype} {tuple(gt.shape)}")
        dev = device("localisation")
        gt = gt.detach().to(device=dev, dtype=torch.float64)
        Rg, tg = gt[:, :3, :3].contiguous(), gt[:, :3, 3].contiguous()
        ok = result["success"]
        rt, rd = pose_errors(result["retrieval_R"], result["retrieval_t"], Rg, tg, valid=ok)
        mt, md = pose_errors(result["R_c2w"], result["t_c2w"], Rg, tg, valid=ok)
        med = torch.stack([_median(rt, ok).double(), _median(rd, ok), _median(mt, ok).double(), _median(md, ok)])
        host = torch.cat([rt.double(), rd, mt.double(), md, ok.double(), med]).cpu().numpy()   # the one host read
        p = [host[i * Q:(i + 1) * Q] for i in range(5)]
        m = host[5 * Q:]
        return PoseReport(p[4] != 0, p[0].astype(np.float32), p[1], p[2].astype(np.float32), p[3],
                          (np.float32(m[0]), np.float64(m[1]), np.float32(m[2]), np.float64(m[3])))
