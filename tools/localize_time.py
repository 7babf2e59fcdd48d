"""Localisation timing on synthetic data (splatloc_amd/localize.py):

  retrieval  `retrieve` (fused similarity + top-k, one status read) at Replica's size (Q = 900, N = 180, D = 4096, k = 10) and at
             an hloc-sized database (N = 20000), against the reference's formula torch.einsum("id,jd->ij", q, db).topk(k) in the
             same process, inputs on the device;
  driver     Localizer.localize over 900 queries on 180 database frames (5 queries per frame, as Replica's split has them)
             against the per-query loop of INTEGRATION.md §17 / §18 on the same data: a room of 200k key Gaussians, 640 x 480
             frames with ~2000 keypoint pixels, ~500 keypoints per query, the FeatureDecoder of SplatLoc's configuration.

HIP events around each region, one warm-up, the two sides of a comparison interleaved, medians reported:
python tools/localize_time.py > profiles/localize_time.json   (--small: a rehearsal at toy sizes)"""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from splatloc_amd import localize as L  # noqa: E402
from splatloc_amd import matching as M  # noqa: E402
from splatloc_amd import pnp as P  # noqa: E402
from splatloc_amd.decoder import FeatureDecoder  # noqa: E402
from tests.golden.make_golden_matching import look_at, ray_depth, wall_points  # noqa: E402

SMALL = "--small" in sys.argv
REPS = 2 if SMALL else 5
DRIVER_REPS = 1 if SMALL else 3
CAMERA = {"model": "PINHOLE", "width": 640, "height": 480, "params": [320.0, 320.0, 319.5, 239.5]}
CONFIG = {"scene": {"bound": [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]], "voxel_sdf": 0.06},
          "decoder": {"enc": "HashGrid", "hidden_dim": 128, "num_layers": 4, "final_dim": 256}}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def retrieval_row(Q, N, D, k, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn((Q, D), generator=g), dim=1).cuda()
    db = torch.nn.functional.normalize(torch.randn((N, D), generator=g), dim=1).cuda()
    ref = lambda: torch.einsum("id,jd->ij", q, db).topk(k, dim=1, largest=True)  # noqa: E731
    ours = lambda: L.retrieve(q, db, k=k)  # noqa: E731
    ours(), ref()
    t_ours, t_ref = [], []
    for _ in range(REPS):
        (idx, _), a = timed(ours)
        (_, ind1), b = timed(ref)
        t_ours.append(a)
        t_ref.append(b)
    lib = L._native.load()
    return {"Q": Q, "N": N, "D": D, "k": k, "retrieve_ms": round(statistics.median(t_ours), 4),
            "torch_einsum_topk_ms": round(statistics.median(t_ref), 4),
            "ratio_torch_over_retrieve": round(statistics.median(t_ref) / statistics.median(t_ours), 3),
            "same_indices_share": round(float((idx == ind1).double().mean()), 6),
            "workspace_bytes": int(lib.splatraster_retrieval_workspace_bytes(Q, N, D, k)), "similarity_matrix_bytes": 4 * Q * N}


def driver_scene(n_points, n_frames, per_frame, n_kp_pixels, n_query_kp, seed=0):
    rng = np.random.default_rng(seed)
    W, H = CAMERA["width"], CAMERA["height"]
    K = np.array([[320.0, 0.0, 319.5], [0.0, 320.0, 239.5], [0.0, 0.0, 1.0]])
    pts = wall_points(rng, n_points).astype(np.float32)
    marker = rng.uniform(0.006, 0.02, size=(n_points, 1)).astype(np.float32)
    frames, poses = [], []
    for f in range(n_frames):
        a = 2 * np.pi * f / n_frames
        eye = np.array([3.0 + 1.2 * np.cos(a), 2.5 + 1.0 * np.sin(a), 1.4])
        c2w = look_at(eye, eye + np.array([np.cos(a + 0.4), np.sin(a + 0.4), -0.05]))
        poses.append(c2w)
        c32 = c2w.astype(np.float32)
        frames.append({"K": K, "c2w": torch.from_numpy(c32),
                       "w2c": torch.from_numpy(np.linalg.inv(c32.astype(np.float64)).astype(np.float32)),
                       "depth": torch.from_numpy(ray_depth(c32.astype(np.float64), K, W, H).astype(np.float32)).cuda(),
                       "sp_kp_mask": torch.from_numpy((rng.random((H, W)) < n_kp_pixels / (W * H)).astype(np.int32)).cuda()})
    torch.manual_seed(0)
    decoder = FeatureDecoder(CONFIG).cuda()
    with torch.no_grad():
        p = decoder.encoding.params
        p.copy_((torch.rand(p.shape, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(p.device))
    pts_d, marker_d = torch.from_numpy(pts).cuda(), torch.from_numpy(marker).cuda()
    queries, db_index, gt = [], [], []
    for f in range(n_frames):
        with torch.no_grad():
            p3, f3, _ = M.get_frusm_pts(pts_d, marker_d, frames[f], K, W, H, decoder)
        for _ in range(per_frame):
            c2w = poses[f].copy()
            c2w[:3, 3] += rng.uniform(-0.1, 0.1, size=3)
            w2c = np.linalg.inv(c2w)
            pc = p3.astype(np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
            uv = pc[:, :2] / pc[:, 2:] * 320.0 + np.array([319.5, 239.5])
            vis = np.flatnonzero((pc[:, 2] > 0.1) & (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H))
            pick = rng.permutation(vis)[:n_query_kp * 4 // 5]
            nd = n_query_kp - len(pick)
            kp = np.concatenate([uv[pick] + rng.normal(size=(len(pick), 2)) * 0.5, rng.uniform(0, [W, H], size=(nd, 2))])
            desc = np.concatenate([f3.cpu().numpy()[pick] + 0.02 * rng.standard_normal((len(pick), 256)).astype(np.float32),
                                   rng.standard_normal((nd, 256)).astype(np.float32)])
            queries.append({"keypoints": kp.astype(np.float32), "descriptors": np.ascontiguousarray(desc.T.astype(np.float32))})
            db_index.append(f)
            gt.append(c2w)
    return pts_d, marker_d, frames, decoder, K, queries, db_index, np.stack(gt)


def per_query_loop(pts, marker, frames, decoder, K, queries, db_index):
    W, H = CAMERA["width"], CAMERA["height"]
    out = []
    with torch.no_grad():
        for q, f in zip(queries, db_index):
            p3, f3, _ = M.get_frusm_pts(pts, marker, frames[f], K, W, H, decoder)
            if p3.shape[0] < 5:
                out.append(None)
                continue
            m = M.HungarianMatcher()({"query_descs": torch.from_numpy(q["descriptors"]), "train_descs": f3.T})["matches"].numpy()
            mq, m3 = q["keypoints"][m[0]], p3[m[1]]
            keep = m3[:, 2] > -10000
            out.append(P.solve_pose(mq[keep], m3[keep], CAMERA))
    return out


def driver_row():
    sizes = (20000, 6, 2, 300, 60) if SMALL else (200000, 180, 5, 2000, 500)
    pts, marker, frames, decoder, K, queries, db_index, gt = driver_scene(*sizes)
    loc = L.Localizer(pts, marker, decoder, K, CAMERA["width"], CAMERA["height"], CAMERA)
    batch = lambda: loc.localize(queries, frames, db_index)  # noqa: E731
    loop = lambda: per_query_loop(pts, marker, frames, decoder, K, queries, db_index)  # noqa: E731
    batch()
    per_query_loop(pts, marker, frames, decoder, K, queries[:3], db_index[:3])
    t_batch, t_loop = [], []
    for _ in range(DRIVER_REPS):
        res, a = timed(batch)
        single, b = timed(loop)
        t_batch.append(a)
        t_loop.append(b)
    R, t, ok = res["R_c2w"].cpu(), res["t_c2w"].cpu(), res["success"].cpu()
    same = all((s is not None and s[2]["success"]) == bool(ok[i]) and
               (not bool(ok[i]) or (torch.equal(R[i], torch.from_numpy(s[0])) and torch.equal(t[i], torch.from_numpy(s[1]))))
               for i, s in enumerate(single))
    rep = loc.evaluate(res, gt)
    return {"queries": len(queries), "frames": len(frames), "key_gaussians": sizes[0], "keypoints_per_query": sizes[4],
            "candidates_per_frame_median": int(np.median([loc._candidates(f, pts.device)[0].shape[0] for f in frames[:8]])),
            "localize_ms": round(statistics.median(t_batch), 2), "per_query_loop_ms": round(statistics.median(t_loop), 2),
            "ratio_loop_over_localize": round(statistics.median(t_loop) / statistics.median(t_batch), 3),
            "bit_identical_to_loop": bool(same), "successes": int(ok.sum()),
            "median_match_cm": round(float(rep.median_match_dist) * 100, 4), "median_match_deg": round(float(rep.median_match_theta), 5)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("localize_time needs the GPU")
    rows = [retrieval_row(64, 180, 256, 10, 1)] if SMALL else [retrieval_row(900, 180, 4096, 10, 1), retrieval_row(900, 20000, 4096, 10, 2)]
    print(json.dumps({
        "what": "localisation (HIP) on MI355X, synthetic data; HIP events around each region after one warm-up, the two sides of a "
                f"comparison interleaved, medians of {REPS} (retrieval) / {DRIVER_REPS} (driver) runs; retrieve_ms includes its "
                "status read; per_query_loop_ms = get_frusm_pts + HungarianMatcher + solve_pose per query",
        "retrieval": rows, "driver": None if "--retrieval-only" in sys.argv else driver_row()}, indent=1))


if __name__ == "__main__":
    main()
