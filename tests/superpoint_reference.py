"""CPU restatement of the SuperPoint head (splatloc_amd/superpoint.py, csrc/superpoint_head.hip) in torch operators, a float64
oracle of its two floating-point rules, seeded case builders and deliberately wrong models.

hloc's SuperPoint is not in the reference tree, so include/splatraster.h (splatraster_sp_*) and INTEGRATION.md §24 are the
contract; this file restates them with the operators the hloc model uses (softmax, max_pool2d, nonzero, grid_sample, normalize)
and a stable sort in place of topk, which carries the tie rule: descending score, equal scores by ascending row-major index.

A case is a dict: "semi" [B,65,Hc,Wc] or a hand-made score map "S" [B,H,W] or suppressed map "N" [B,H,W], optionally "coarse"
[B,256,Hc,Wc], and the parameters r, thr, K, border.  `head(case, wrong=None)` runs the stages the case has inputs for and
returns padded outputs shaped like the device's.  WRONG names the mutations; each must change the output of at least one case
(tests/test_host_superpoint_head.py), or the cases would not pin the rule it breaks.
"""
import numpy as np
import torch
import torch.nn.functional as F

CELL = 8
EPS = 1e-12

WRONG = ("rounds_0", "rounds_1", "rounds_3", "zero_pad_pool", "channel_order", "threshold_ge", "border_low", "border_high",
         "always_sorted", "ties_descending", "align_corners_false", "offset_dropped", "border_padding", "second_norm_dropped")


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def scores(semi, wrong=None):
    """S [B,8Hc,8Wc]: softmax over the 65 channels, dustbin dropped, S[b, 8i+u, 8j+v] = p[b, 8u+v, i, j]"""
    b, _, hc, wc = semi.shape
    p = F.softmax(semi, 1)[:, :-1]
    p = p.permute(0, 2, 3, 1).reshape(b, hc, wc, CELL, CELL)          # [b, i, j, u, v]
    if wrong == "channel_order":
        p = p.transpose(3, 4)                                          # channel 8v + u
    return p.permute(0, 1, 3, 2, 4).reshape(b, hc * CELL, wc * CELL).contiguous()


def scores64(semi):
    return scores(semi.double())


def _pool(x, r, zero_pad=False):
    if zero_pad:
        return F.max_pool2d(F.pad(x, (r, r, r, r), value=0.0), 2 * r + 1, stride=1)
    return F.max_pool2d(x, 2 * r + 1, stride=1, padding=r)


def nms(S, r, wrong=None):
    """N [B,H,W]: M0 = (S == pool(S)); twice: Supp = pool(M) > 0, Q = where(Supp, 0, S), M |= (Q == pool(Q)) & ~Supp"""
    if r == 0:
        return S.clone()
    rounds = {"rounds_0": 0, "rounds_1": 1, "rounds_3": 3}.get(wrong, 2)
    zeros = torch.zeros_like(S)
    M = S == _pool(S, r, wrong == "zero_pad_pool")
    for _ in range(rounds):
        supp = _pool(M.float(), r) > 0
        Q = torch.where(supp, zeros, S)
        M = M | ((Q == _pool(Q, r)) & ~supp)
    return torch.where(M, S, zeros)


def select(N, thr, K, border, wrong=None):
    """(keypoints [B,K,2] (x, y), scores [B,K], count [B], candidates [B]), rows at and beyond count zero"""
    B, H, W = N.shape
    thr = torch.tensor(thr, dtype=torch.float32)
    kps, scs = torch.zeros(B, K, 2), torch.zeros(B, K)
    count, cand = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    rows, cols = torch.arange(H)[:, None], torch.arange(W)[None, :]
    lo = border + 1 if wrong == "border_low" else border
    hi = border - 1 if wrong == "border_high" else border
    inside = (rows >= lo) & (rows < H - hi) & (cols >= lo) & (cols < W - hi)
    for b in range(B):
        ok = ((N[b] >= thr) if wrong == "threshold_ge" else (N[b] > thr)) & inside
        rc = torch.nonzero(ok)                                         # row-major
        s = N[b][rc[:, 0], rc[:, 1]]
        n = len(s)
        if n > K or wrong == "always_sorted":
            if wrong == "ties_descending":
                order = torch.sort(s.flip(0), descending=True, stable=True)[1]
                order = (n - 1 - order)[:K]
            else:
                order = torch.sort(s, descending=True, stable=True)[1][:K]
            rc, s = rc[order], s[order]
        m = min(n, K)
        kps[b, :m] = rc[:m].flip(1).float()
        scs[b, :m] = s[:m]
        count[b], cand[b] = m, n
    return kps, scs, count, cand


def grid_coords(kp, hc, wc, wrong=None):
    """(ix, iy) of keypoints [..., 2] in float32, in exactly the contract's steps"""
    dt = kp.dtype
    off = 0.0 if wrong == "offset_dropped" else 3.5
    size = torch.tensor([CELL * wc - 4.5, CELL * hc - 4.5], dtype=dt)
    g = ((kp - off) / size) * 2 - 1
    cells = torch.tensor([wc, hc], dtype=dt)
    if wrong == "align_corners_false":
        return g, ((g + 1) * cells - 1) / 2
    return g, ((g + 1) / 2) * (cells - 1)


def sample(coarse, kp, count, wrong=None):
    """descriptors [B,256,K] at keypoints [B,K,2]; columns at and beyond count zero"""
    B, C, hc, wc = coarse.shape
    K = kp.shape[1]
    d = F.normalize(coarse, p=2, dim=1, eps=EPS)
    g, _ = grid_coords(kp, hc, wc, wrong)
    out = F.grid_sample(d, g.view(B, 1, K, 2), mode="bilinear", align_corners=wrong != "align_corners_false",
                        padding_mode="border" if wrong == "border_padding" else "zeros").reshape(B, C, K)
    if wrong != "second_norm_dropped":
        out = F.normalize(out, p=2, dim=1, eps=EPS)
    live = torch.arange(K)[None, :] < count[:, None]
    return torch.where(live[:, None, :], out, torch.zeros_like(out))


def sample64(coarse, kp, count):
    return sample(coarse.double(), kp.double(), count)


def floors(kp, hc, wc):
    """floor(ix), floor(iy) of keypoints [B,K,2] in float32: [B,K,2]"""
    return torch.floor(grid_coords(kp, hc, wc)[1])


def dense(coarse, rows=None):
    """[B,rows,W,256]: `sample` at every pixel"""
    B, _, hc, wc = coarse.shape
    H, W = CELL * hc, CELL * wc
    r0, r1 = (0, H) if rows is None else rows
    ys, xs = torch.meshgrid(torch.arange(r0, r1, dtype=coarse.dtype), torch.arange(W, dtype=coarse.dtype), indexing="ij")
    kp = torch.stack([xs, ys], -1).reshape(1, -1, 2).expand(B, -1, -1)
    d = sample(coarse, kp, torch.full((B,), kp.shape[1], dtype=torch.int32))
    return d.permute(0, 2, 1).reshape(B, r1 - r0, W, 256).contiguous()


def head(case, wrong=None):
    """every stage the case has inputs for, with the device's padded shapes"""
    out = {}
    if "N" in case:
        N = case["N"]
    else:
        S = case["S"] if "S" in case else scores(case["semi"], wrong)
        out["S"] = S
        N = nms(S, case["r"], wrong)
    out["N"] = N
    kp, sc, count, cand = select(N, case["thr"], case["K"], case["border"], wrong)
    out.update(keypoints=kp, scores=sc, count=count, candidates=cand)
    if "coarse" in case:
        out["descriptors"] = sample(case["coarse"], kp, count, wrong)
    return out


def same(a, b):
    """bit-for-bit equality of two `head` results (NaN-free)"""
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


# ---- cases -----------------------------------------------------------------------------------------------------------------------

def _params(r=4, thr=0.005, K=4096, border=4):
    return {"r": r, "thr": thr, "K": K, "border": border}


def random_case(hc, wc, B=1, seed=0, **kw):
    """normal logits and normal coarse features"""
    g = torch.Generator().manual_seed(seed)
    return {"semi": torch.randn(B, 65, hc, wc, generator=g), "coarse": torch.randn(B, 256, hc, wc, generator=g), **_params(**kw)}


def peaked_case(hc, wc, B=1, seed=0, **kw):
    """logits three times as wide: scores spread over decades, as a trained head's do, so the threshold cuts among them"""
    c = random_case(hc, wc, B, seed, **kw)
    c["semi"] = c["semi"] * 3.0
    return c


def two_counts_case(seed=5):
    """B = 2: image 0 has many candidates, image 1 a flat dustbin-dominated map with few"""
    c = peaked_case(5, 9, 2, seed, K=20)
    c["semi"][1, 64] += 14.0
    return c


def plateau_case(seed=7):
    """one cell whose 64 logits are equal and dominate the neighbourhood: an 8 x 8 plateau of equal scores, all of which survive"""
    c = random_case(5, 9, 1, seed, border=0)
    c["semi"][0, 64] += 8.0                      # every other cell: scores well below 1 / 64
    c["semi"][0, :64, 2, 4] = 4.0
    c["semi"][0, 64, 2, 4] = -4.0
    return c


def chain_map(H, W, start, step, length, base=0.9, seed=11):
    """a score map [1,H,W] of small noise with `length` maxima, 3 px apart from `start` (row, col) along `step`, descending"""
    g = torch.Generator().manual_seed(seed)
    S = torch.rand(1, H, W, generator=g) * 1e-3
    for k in range(length):
        S[0, start[0] + 3 * k * step[0], start[1] + 3 * k * step[1]] = base - 0.01 * k
    return S


def chain_case(H=24, W=32, start=(11, 1), step=(0, 1), length=8, seed=11):
    """0 / 1 / 2 / 3 extra rounds keep the first 1 / 2 / 3 / 4 of every second maximum (columns 1, 7, 13, 19 for the default):
    the contract's two rounds keep three"""
    g = torch.Generator().manual_seed(seed + 1)
    return {"S": chain_map(H, W, start, step, length, seed=seed), "coarse": torch.randn(1, 256, H // CELL, W // CELL, generator=g),
            **_params(thr=0.5, border=0)}


def tile_chain_cases(tile_h, tile_w):
    """chains laid across a tile's vertical edge, across its horizontal edge, and one ending in the image corner"""
    H, W = tile_h + CELL, tile_w + 2 * CELL
    return {"chain_vertical_edge": chain_case(H, W, (tile_h // 2, tile_w - 11), (0, 1), 8, seed=21),
            "chain_horizontal_edge": chain_case(H, W, (tile_h - 11, tile_w // 2), (1, 0), 6, seed=22),
            "chain_corner": chain_case(H, W, (H - 1, W - 1 - 21), (0, 1), 8, seed=23)}


def negative_map_case(seed=13):
    """negative scores through `nms`: a clipped window and a zero-padded one disagree along the image edge"""
    g = torch.Generator().manual_seed(seed)
    return {"S": -torch.rand(1, 24, 32, generator=g) - 0.1, "coarse": torch.randn(1, 256, 3, 4, generator=g), **_params(thr=0.0, border=0)}


def _empty_map(H=24, W=32):
    return torch.zeros(1, H, W)


def threshold_case():
    """a score equal to the float32 threshold and its two neighbours by nextafter: only the upper one is a candidate"""
    t = np.float32(0.005)
    N = _empty_map()
    N[0, 10, 5], N[0, 10, 15], N[0, 10, 25] = float(np.nextafter(t, np.float32(0))), float(t), float(np.nextafter(t, np.float32(1)))
    return {"N": N, **_params(thr=float(t), border=0)}


def count_case(extra, K=12, seed=17):
    """n = K + extra distinct scores scattered in no order: n <= K keeps the row-major order, n = K + 1 switches to descending"""
    g = torch.Generator().manual_seed(seed)
    N = _empty_map()
    at = torch.randperm(24 * 32, generator=g)[:K + extra]
    N.view(-1)[at] = torch.rand(K + extra, generator=g) * 0.5 + 0.1
    return {"N": N, **_params(K=K, border=0)}


def ties_case(K=10):
    """n > K with equal scores straddling the cut: four above it, then nine equal ones of which the six with the smallest
    row-major index stay"""
    N = _empty_map()
    for k in range(4):
        N[0, 20 - 5 * k, 3 + 7 * k] = 0.9 - 0.1 * k
    for k in range(9):
        N[0, 2 + 2 * k, 30 - 3 * k] = 0.25
    return {"N": N, **_params(K=K, border=0)}


def none_case():
    return {"N": _empty_map(), **_params(border=0)}


def every_pixel_case(border, seed=19):
    """every pixel a candidate (r = 0, threshold 0, K = 64 on 24 x 32), with the given border"""
    c = random_case(3, 4, 1, seed, r=0, thr=0.0, K=64, border=border)
    return c


def descriptor_edge_case(seed=23):
    """border 0 with keypoints at (0, 0), (W - 1, H - 1), (3, 3) and (4, 4) on 3 x 4 cells: the zero padding is live at the first two"""
    g = torch.Generator().manual_seed(seed)
    N = _empty_map()
    for x, y in ((0, 0), (31, 23), (3, 3), (4, 4)):
        N[0, y, x] = 0.5
    return {"N": N, "coarse": torch.randn(1, 256, 3, 4, generator=g), **_params(border=0)}


def host_cases(tile=(64, 64)):
    cases = {"cells_3x4": peaked_case(3, 4, 1, 1), "cells_5x9": peaked_case(5, 9, 1, 2),
             "over_a_tile": peaked_case(tile[0] // CELL + 1, tile[1] // CELL + 1, 1, 3, K=50),
             "normal_3x4_b2": random_case(3, 4, 2, 4), "chain": chain_case(), "plateau": plateau_case(), "two_counts": two_counts_case(),
             "negative_map": negative_map_case(), "threshold": threshold_case(), "count_K": count_case(0), "count_K_plus_1": count_case(1),
             "ties": ties_case(), "none": none_case(), "every_pixel_b0": every_pixel_case(0), "every_pixel_b4": every_pixel_case(4),
             "every_pixel_b12": every_pixel_case(12), "descriptor_edges": descriptor_edge_case()}
    cases.update(tile_chain_cases(*tile))
    return cases
