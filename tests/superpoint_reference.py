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


def negative_map_case(seed=13, H=24, W=32, r=4):
    """negative scores through `nms`: a clipped window and a zero-padded one disagree along the image edge; 72 x 88 crosses the
    edges of both tile sizes"""
    g = torch.Generator().manual_seed(seed)
    return {"S": -torch.rand(1, H, W, generator=g) - 0.1, "coarse": torch.randn(1, 256, H // CELL, W // CELL, generator=g),
            **_params(r=r, thr=0.0, border=0)}


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


# ---- edges: the device algorithm restated ----------------------------------------------------------------------------------------
# What follows models how csrc/superpoint_head.hip computes, with its constants, where it differs from the restatement above: NMS
# on tiles with a halo, selection through chunks, digit passes, a stepped walk and ranks counted over tiles.  Each model equals
# the contract; each of its defects (NMS_TILED_WRONG, SELECT_MODEL_WRONG) changes at least one edge case
# (tests/test_host_superpoint_edges.py), so the cases that run on the device (tests/test_gpu_superpoint_edges.py) pin that code.

EDGE = 64                        # an edge of both NMS tile sizes (64 up to r = 4, 32 above)
RADII = tuple(range(1, 9))
NMS_TILED_WRONG = ("panel_zero_pad", "outside_zero", "suppression_unclipped", "halo_of_64_tile")
SEL_CHUNK, SEL_ITEMS, PICK_STEP, RANK_TILE, RANK_GROUP = 2048, 8, 1024, 1024, 256
SELECT_MODEL_WRONG = ("eq_carry_dropped", "sel_carry_dropped", "ties_without_tile_offset", "pads_counted", "digits_ascending",
                      "one_equal_too_many", "offsets_stride", "lane_rows")


def nms_tile_of(r):
    return 64 if r <= 4 else 32


def _explicit_panel(S, inside, r, wrong):
    """`nms` of a panel that reaches beyond the image, as the kernel computes it: pixels outside (`inside` false) are -inf for the
    float maxima and 0 for the masks, windows are clipped at the panel's edge"""
    out_val = 0.0 if wrong == "outside_zero" else float("-inf")
    zeros, outside = torch.zeros_like(S), torch.full_like(S, out_val)
    X = torch.where(inside, S, outside)
    M = (X == _pool(X, r)) & inside
    for _ in range(2):
        supp = _pool((M | ~inside if wrong == "suppression_unclipped" else M).float(), r) > 0
        Q = torch.where(inside, torch.where(supp, zeros, X), outside)
        M = M | ((Q == _pool(Q, r)) & ~supp & inside)
    return torch.where(M, S, zeros)


def _zero_pad_panel(S, r):
    """`nms` of a panel whose float maxima see 0 beyond the panel's edge"""
    zeros = torch.zeros_like(S)
    M = S == _pool(S, r, True)
    for _ in range(2):
        supp = _pool(M.float(), r) > 0
        Q = torch.where(supp, zeros, S)
        M = M | ((Q == _pool(Q, r, True)) & ~supp)
    return torch.where(M, S, zeros)


def nms_tiled(S, r, tile, halo, wrong=None):
    """N [B,H,W] as sp_nms_kernel computes it: every tile x tile block of outputs from its own panel, the block plus `halo` pixels
    on each side clipped to the image, by `nms` with the panel's edge as a window clip.  The device's halo is 5 r.
    wrong: "panel_zero_pad" the float maxima read 0 beyond a panel's edge, "outside_zero" the panel is not clipped and its pixels
    outside the image read 0 in the float maxima (the kernel's -inf), "suppression_unclipped" the panel is not clipped and the window of Supp reads
    the mask as set outside the image (the kernel's 0), so every pixel within r of the image's edge is suppressed,
    "halo_of_64_tile" the 32-pixel tile with the halo the 64-pixel tile's panel has room for (at most 20)"""
    B, H, W = S.shape
    if wrong == "halo_of_64_tile" and tile == 32:
        halo = min(halo, 5 * 4)
    out = torch.empty_like(S)
    for y0 in range(0, H, tile):
        for x0 in range(0, W, tile):
            y1, x1 = min(y0 + tile, H), min(x0 + tile, W)
            if wrong in ("outside_zero", "suppression_unclipped"):
                ys, xs = torch.arange(y0 - halo, y0 + tile + halo), torch.arange(x0 - halo, x0 + tile + halo)
                inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
                panel = S[:, ys.clamp(0, H - 1)][:, :, xs.clamp(0, W - 1)]
                n = _explicit_panel(panel, inside[None].expand_as(panel), r, wrong)
                out[:, y0:y1, x0:x1] = n[:, halo:halo + y1 - y0, halo:halo + x1 - x0]
                continue
            py, px = max(y0 - halo, 0), max(x0 - halo, 0)
            panel = S[:, py:min(y0 + tile + halo, H), px:min(x0 + tile + halo, W)]
            n = _zero_pad_panel(panel, r) if wrong == "panel_zero_pad" else nms(panel, r)
            out[:, y0:y1, x0:x1] = n[:, y0 - py:y1 - py, x0 - px:x1 - px]
    return out


def reach_chains(r):
    """the five chains of `reach_case(r)`: (image, decisive pixel (row, col), direction (drow, dcol) from the head towards it)"""
    E = EDGE
    return ((0, (20, E), (0, 1)), (0, (45, E - 1), (0, -1)), (1, (E, 20), (1, 0)), (1, (E - 1, 45), (-1, 0)), (0, (E, E), (1, 1)))


def reach_case(r, heads=True, seed=29):
    """S [2,131,137] of small noise with five chains of seven maxima r apart: a head of 0.95, then 0.9 - 0.01 k for k = 0..5, the
    fifth of them (k = 4) on the chain's decisive pixel, 5 r from the head.  The head wins round 0, k = 1 round 1 and k = 3 round 2,
    so the decisive pixel loses; without the head (heads=False) k = 0, 2, 4 win and it survives.  Its result therefore depends on S
    exactly 5 r away.  Four chains run along a row or a column and end on column / row EDGE (from the left / from above) or
    EDGE - 1 (from the right / from below), the first and the last pixel of a tile at both tile sizes; the fifth runs diagonally
    onto (EDGE, EDGE), through the corner of the halo."""
    g = torch.Generator().manual_seed(seed + r)
    S = torch.rand(2, 131, 137, generator=g) * 1e-3
    for b, (y, x), (dy, dx) in reach_chains(r):
        if heads:
            S[b, y - 5 * r * dy, x - 5 * r * dx] = 0.95
        for k in range(6):
            S[b, y - (4 - k) * r * dy, x - (4 - k) * r * dx] = 0.9 - 0.01 * k
    return {"S": S, **_params(r=r, thr=0.5, K=64, border=0)}


def quantised_map(levels, seed=37, B=2, H=131, W=137):
    """a map of `levels` values: plateaus of equal scores across every tile edge"""
    g = torch.Generator().manual_seed(seed)
    return torch.floor(torch.rand(B, H, W, generator=g) * levels) / levels


def nms_edge_maps():
    """name -> (S, r): what the device NMS is held to beyond the reach cases"""
    g = torch.Generator().manual_seed(43)
    maps = {"negative_r3": (negative_map_case(47, 72, 88, 3)["S"], 3), "negative_r6": (negative_map_case(53, 72, 88, 6)["S"], 6),
            "quantised_r2": (quantised_map(4), 2), "quantised_r7": (quantised_map(4, seed=41), 7)}
    for r in (4, 8):
        for shape in ((1, 1, 1), (1, 1, 200), (1, 200, 1), (3, 5, 7), (1, 64, 64), (1, 65, 65)):
            maps["x".join(map(str, shape)) + f"_r{r}"] = (torch.rand(*shape, generator=g), r)
    return maps


# selection: hand-made N maps

def _scatter(B, H, W, counts, g, lo=0.1, hi=0.9):
    """N [B,H,W]: image b holds counts[b] distinct scores in (lo, hi) at scattered pixels, zero elsewhere"""
    N = torch.zeros(B, H, W)
    for b, n in enumerate(counts):
        at = torch.randperm(H * W, generator=g)[:n]
        N[b].view(-1)[at] = lo + (hi - lo) * (torch.randperm(n, generator=g) + 1).float() / (n + 1)
    return N


def production_k_case(seed=61):
    """every pixel of [2,96,128] a distinct positive score, K = 4096: n = 12288 is twelve steps of the pick walk, K is sixteen rank
    groups and four rank tiles"""
    g = torch.Generator().manual_seed(seed)
    N = torch.stack([(torch.randperm(12288, generator=g) + 1).float() / 16384 for _ in range(2)]).view(2, 96, 128)
    return {"N": N, **_params(thr=0.0, K=4096, border=0)}


def long_ties_case(seed=67):
    """five score classes on [2,96,128]; the cut at K = 4096 falls inside the 0.5 class, whose members lie all over the list"""
    g = torch.Generator().manual_seed(seed)
    N = torch.floor(torch.rand(2, 96, 128, generator=g) * 5) / 8 + 0.125
    return {"N": N, **_params(thr=0.0, K=4096, border=0)}


def shared_digits_case(low_byte=None, seed=71):
    """keys 0x3F000000 + j with distinct j < 65536 on [1,96,128]: the two upper digit passes see one bin.  low_byte: K is the first
    one from 1100 up whose K-th largest key ends in that byte (0x00: the cut is the last of its bin, 0xFF: the first)"""
    g = torch.Generator().manual_seed(seed)
    j = torch.randperm(65536, generator=g)[:12288].numpy().astype(np.uint32)
    desc = np.sort(j)[::-1]
    K = 1100
    if low_byte is not None:
        K = 1100 + int(np.nonzero((desc[1099:] & 255) == low_byte)[0][0])
    N = torch.from_numpy((np.uint32(0x3F000000) + j).view(np.float32).reshape(1, 96, 128).copy())
    return {"N": N, **_params(thr=0.0, K=K, border=0)}


def k_edge_case(K, n, seed=73):
    """n distinct scores scattered over [1,48,80] with max_keypoints = K"""
    g = torch.Generator().manual_seed(seed + K + n)
    return {"N": _scatter(1, 48, 80, [n], g), **_params(K=K, border=0)}


def largest_k_case(seed=79):
    """K = 65535, every pixel of [1,264,256] a candidate: n = 67584 (float32 rand: a few hundred equal pairs among them)"""
    g = torch.Generator().manual_seed(seed)
    return {"N": torch.rand(1, 264, 256, generator=g) * 0.5 + 0.25, **_params(thr=0.0, K=65535, border=0)}


def ragged_case(K, seed=83):
    """[2,37,61] with border 3, every pixel above the threshold: W is odd, so a lane's eight pixels straddle rows, the last chunk
    is ragged (2257 = 2048 + 209 pixels) and the border rule is worked out from a flat index"""
    g = torch.Generator().manual_seed(seed)
    return {"N": torch.rand(2, 37, 61, generator=g) * 0.5 + 0.25, **_params(thr=0.0, K=K, border=3)}


def many_chunks_case():
    """[2,1025,2048]: 1025 chunks per image, two steps of the scan over the chunk counts; five candidates in all"""
    N = torch.zeros(2, 1025, 2048)
    N[0, 0, 5], N[0, 1023, 2047], N[0, 1024, 0] = 0.5, 0.75, 0.25
    N[1, 512, 7], N[1, 1024, 2047] = 0.625, 0.375
    return {"N": N, **_params(K=4, border=0)}


def mixed_batch_case(seed=89):
    """B = 5 with n = 0, n < K, n = K, n = K + 1 and n = 8 K at K = 300 in one call"""
    g = torch.Generator().manual_seed(seed)
    return {"N": _scatter(5, 48, 80, [0, 100, 300, 301, 2400], g), **_params(K=300, border=0)}


def select_edge_cases(large=True):
    """name -> case with "N"; large: with the two cases of millions of pixels or K^2 = 4 10^9"""
    cases = {"production_k": production_k_case(), "long_ties": long_ties_case(), "shared_digits": shared_digits_case(),
             "shared_digits_low_00": shared_digits_case(0x00), "shared_digits_low_ff": shared_digits_case(0xFF),
             "ragged_listed": ragged_case(4096), "ragged_ranked": ragged_case(300), "mixed_batch": mixed_batch_case()}
    for K in (1, 256, 257, 1024, 1025):
        cases[f"k{K}_plus_1"] = k_edge_case(K, K + 1)
        cases[f"k{K}_times_3"] = k_edge_case(K, 3 * K)
    if large:
        cases["largest_k"] = largest_k_case()
        cases["many_chunks"] = many_chunks_case()
    return cases


def _excl(v):
    return np.cumsum(v) - v


def select_device_model(N, thr, K, border, wrong=None, trace=None):
    """`select` as the device computes it (sp_compact_kernel, sp_offsets_kernel, sp_pick_kernel, sp_rank_kernel), in numpy:
    chunks of 2048 pixels with eight consecutive pixels per lane and the row and column of a pixel from its flat index; the chunk
    counts scanned per image in steps of 1024 with a running total; for n > K four 8-bit digit passes from the top for the K-th
    largest key T and the number k of keys equal to T still needed, a walk over the list in steps of 1024 with the running counts
    of equal and of selected keys, and the place of survivor i as (larger keys) + (equal keys in front of it), counted over tiles
    of 1024 whose pads are 0 and where `before` = clamp(i - j0, 0, 1024) entries of the tile at j0 lie in front of i.
    Same outputs as `select`.  trace: a dict that receives per image the steps taken (for the tests of the builders).
    wrong (SELECT_MODEL_WRONG): "eq_carry_dropped" / "sel_carry_dropped" the walk forgets a running count between steps,
    "ties_without_tile_offset" `before` from i, not i - j0, "pads_counted" a tile's pads count as ties in front,
    "digits_ascending" a digit's bins walked from 0 up, "one_equal_too_many" k + 1 of the keys equal to T kept,
    "offsets_stride" image b's chunk counts scanned at b (chunks - 1), "lane_rows" a lane's eight pixels all placed in the row of
    its first one, as if W were a multiple of 8"""
    B, H, W = N.shape
    pixels = H * W
    chunks = -(-pixels // SEL_CHUNK)
    val = N.reshape(B, pixels).numpy()
    thr = np.float32(thr)
    kps, scs = np.zeros((B, K, 2), np.float32), np.zeros((B, K), np.float32)
    count, cand = np.zeros(B, np.int32), np.zeros(B, np.int32)

    # sp_compact_kernel<false>: one count per chunk
    p = np.arange(chunks * SEL_CHUNK, dtype=np.int64)
    if wrong == "lane_rows":
        p0 = p - p % SEL_ITEMS
        row = p0 // W
        col = p0 - row * W + p % SEL_ITEMS
    else:
        row = p // W
        col = p - row * W
    ok_place = (p < pixels) & (row >= border) & (row < H - border) & (col >= border) & (col < W - border)
    flags = np.zeros((B, chunks * SEL_CHUNK), bool)
    flags[:, :pixels] = val > thr
    flags &= ok_place[None]
    counts = flags.reshape(B * chunks, SEL_CHUNK).sum(1).astype(np.int64)

    # sp_offsets_kernel: image b's counts become their exclusive scan, in place
    stride = chunks - 1 if wrong == "offsets_stride" else chunks
    for b in range(B):
        c = counts[b * stride:b * stride + chunks]
        run = 0
        for i0 in range(0, chunks, PICK_STEP):
            v = c[i0:i0 + PICK_STEP].copy()
            c[i0:i0 + PICK_STEP] = run + _excl(v)
            run += int(v.sum())
        cand[b], count[b] = run, min(run, K)

    for b in range(B):
        # sp_compact_kernel<true>: (key, pixel) in row-major order, chunk by chunk
        ckey, cidx = np.zeros(pixels, np.uint32), np.zeros(pixels, np.uint32)
        f = flags[b].reshape(chunks, SEL_CHUNK)
        for ch in np.nonzero(f.any(1))[0]:
            at = np.nonzero(f[ch])[0] + ch * SEL_CHUNK
            pos = counts[b * chunks + ch] + np.arange(len(at))
            fits = pos < pixels
            ckey[pos[fits]] = val[b, at[fits]].view(np.uint32)
            cidx[pos[fits]] = at[fits]
        n = min(int(cand[b]), pixels)
        steps = {"n": n, "pick_steps": 0, "rank_tiles": 0, "rank_groups": 0, "chunks": chunks, "offset_steps": -(-chunks // PICK_STEP)}
        if trace is not None:
            trace[b] = steps

        def write(rows, keys, idxs):
            r_ = idxs // np.uint32(W)
            kps[b, rows, 0], kps[b, rows, 1] = (idxs - r_ * np.uint32(W)).astype(np.float32), r_.astype(np.float32)
            scs[b, rows] = keys.view(np.float32)

        if n <= K:
            write(np.arange(n), ckey[:n], cidx[:n])
            continue

        # sp_pick_kernel: the K-th largest key and how many of its equals are needed
        key = ckey[:n]
        prefix, k = np.uint32(0), K
        for shift in (24, 16, 8, 0):
            hi = np.uint32(0) if shift == 24 else np.uint32((0xFFFFFFFF << (shift + 8)) & 0xFFFFFFFF)
            hist = np.bincount((key[(key & hi) == prefix] >> np.uint32(shift)) & np.uint32(255), minlength=256)
            order = np.arange(256) if wrong == "digits_ascending" else np.arange(255, -1, -1)
            incl = np.cumsum(hist[order])
            at = int(np.searchsorted(incl, k, "left"))            # the first bin whose inclusive count reaches k
            at = min(at, 255)
            k = k - int(incl[at] - hist[order][at])
            prefix = np.uint32(prefix | (np.uint32(order[at]) << np.uint32(shift)))
        steps["T"], steps["k"] = int(prefix), int(k)
        if wrong == "one_equal_too_many":
            k += 1
        okey, oidx = np.zeros(K, np.uint32), np.zeros(K, np.uint32)
        eq_run = sel_run = 0
        for i0 in range(0, n, PICK_STEP):
            u, ix = key[i0:i0 + PICK_STEP], cidx[i0:min(i0 + PICK_STEP, n)]
            eq = u == prefix
            eq_at = eq_run + _excl(eq.astype(np.int64))
            sel = (u > prefix) | (eq & (eq_at < k))
            at = sel_run + _excl(sel.astype(np.int64))
            w = sel & (at < K)
            okey[at[w]], oidx[at[w]] = u[w], ix[w]
            if wrong != "eq_carry_dropped":
                eq_run += int(eq.sum())
            if wrong != "sel_carry_dropped":
                sel_run += int(sel.sum())
            steps["pick_steps"] += 1

        # sp_rank_kernel: lane i of group i / 256 counts over the tiles
        groups = -(-K // RANK_GROUP)
        i = np.arange(groups * RANK_GROUP, dtype=np.int64)
        mine = np.where(i < K, np.concatenate([okey, np.zeros(len(i) - K, np.uint32)]), 0).astype(np.int64)
        rank = np.zeros(len(i), np.int64)
        for j0 in range(0, K, RANK_TILE):
            live = min(K - j0, RANK_TILE)
            s_k = np.zeros(RANK_TILE, np.int64)
            s_k[:live] = okey[j0:j0 + live]
            before = np.clip(i if wrong == "ties_without_tile_offset" else i - j0, 0, RANK_TILE)
            # counted, not compared pairwise: (key, place in the tile) in ascending order
            comp = np.sort(s_k * (2 * RANK_TILE) + np.arange(RANK_TILE))
            larger = RANK_TILE - np.searchsorted(comp, (mine + 1) * (2 * RANK_TILE), "left")
            ties = np.searchsorted(comp, mine * (2 * RANK_TILE) + before, "left") - np.searchsorted(comp, mine * (2 * RANK_TILE), "left")
            rank += larger + ties
            if wrong == "pads_counted":
                rank += RANK_TILE - live
            steps["rank_tiles"] += 1
        steps["rank_groups"] = groups
        w = (i < K) & (rank < K)
        write(rank[w], okey[i[w]], oidx[i[w]])
    return torch.from_numpy(kps), torch.from_numpy(scs), torch.from_numpy(count), torch.from_numpy(cand)


# descriptors and scores

def one_hot_coarse(hc, wc, B=1):
    """one unit vector per cell: the non-zero channels of a descriptor name the cells with a non-zero weight"""
    n = hc * wc
    coarse = torch.zeros(B, 256, hc, wc)
    coarse[:, torch.arange(n), torch.arange(n) // wc, torch.arange(n) % wc] = 1.0
    return coarse


def pixel_keypoints(B, W, rows):
    """keypoints [B,n,2]: every pixel (x, y) of the row range, row-major"""
    ys, xs = torch.meshgrid(torch.arange(rows[0], rows[1], dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys], -1).reshape(1, -1, 2).expand(B, -1, -1).contiguous()


def subpixel_keypoints(hc, wc, n=4096, seed=97):
    """keypoints [1,n,2] at multiples of 1/4 px over [-8, W + 8) x [-8, H + 8), without repetition"""
    g = torch.Generator().manual_seed(seed)
    nx, ny = 4 * (CELL * wc + 16), 4 * (CELL * hc + 16)
    at = torch.randperm(nx * ny, generator=g)[:n]
    return torch.stack([(at % nx).float() / 4 - 8, (at // nx).float() / 4 - 8], -1).view(1, n, 2)


def far_keypoints():
    """([1,32,2], far [32] bool): finite positions far outside the image, mixed with positions inside it in both 16-keypoint groups"""
    kp = torch.tensor([[5.0 + 2 * i, 3.0 + i] for i in range(32)])
    far = {1: (1e6, 10.0), 4: (-1e6, 10.0), 6: (10.0, 1e6), 9: (10.0, -1e6), 12: (3e38, 3e38), 15: (-3e38, 20.0), 16: (20.0, -3e38),
           21: (-3e38, -3e38), 22: (3e38, -1e6), 30: (1e6, 1e6), 31: (-1e6, 3e38)}
    for i, xy in far.items():
        kp[i] = torch.tensor(xy)
    mask = torch.zeros(32, dtype=torch.bool)
    mask[list(far)] = True
    return kp.view(1, 32, 2), mask


def score_edge_cases(seed=101):
    """semi [2,65,5,9]: near one-hot with underflowing tails, all logits equal, a dominant dustbin, logits offset by +-1e4"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(2, 65, 5, 9, generator=g)
    dustbin = base.clone()
    dustbin[:, 64] += 30.0
    offset = base.clone()
    offset[0] += 1e4
    offset[1] -= 1e4
    return {"wide_logits": base * 20.0, "equal_logits": torch.full((2, 65, 5, 9), 0.75), "dustbin_plus_30": dustbin, "offset_1e4": offset}


def decade_errors(got, ref, want):
    """[(top of the decade, device max error, restatement max error, bound)] of float32 maps got and ref against float64 want, per
    decade [top / 10, top) of want, from 1 down to float32's smallest subnormal, and what lies below in a last band.  bound: four
    times the restatement's error, floored at one float32 ulp of the decade's top (the CPU softmax can be exact in a band)"""
    got, ref, want = got.double().flatten(), ref.double().flatten(), want.flatten()
    rows = []
    for d in range(0, 47):
        top, low = 10.0 ** -d, 10.0 ** -(d + 1)
        band = (want < top) & (want >= low) if 0 < d < 46 else (want >= low) if d == 0 else (want < top)
        if not band.any():
            continue
        ulp = float(np.spacing(np.float32(max(top, 1.5e-45))))
        e_got, e_ref = float((got - want)[band].abs().max()), float((ref - want)[band].abs().max())
        rows.append((top, e_got, e_ref, max(4.0 * e_ref, ulp)))
    return rows
