"""Reference, cases, bounds and wrong models for the per-Gaussian projection at its cull, clamp and tile-rect edges: the forward of
csrc/preprocess.hip (preprocess_kernel, plain and raw parameters, one view or a window) and the backward of csrc/projection_bwd.h
(projection_row_bwd + sigma3_chain_bwd) as inlined into preprocess_bwd_kernel, camera_bwd_kernel and window_joint_bwd_kernel.
No GPU import.

  tests/test_host_projection_edges.py   every builder reaches its edge, the CPU oracle (oracle/splat_oracle.c) takes the reference's
                                        decisions and lies within `oracle_bound` of it, every wrong model below exceeds the bound of a
                                        case that names it
  tests/test_gpu_projection_edges.py    the kernels against the reference within the bounds below, through every backward entry point

REFERENCE.  `project()` states the projection of one view in float64 torch (cull, pixel centre, view depth, conic, radius, tile
rectangle, tile count); `reference()` feeds it to tests/torch_dense_ref.render_dense (its `projection=` argument) for the compositing,
sums the loss of every view of a window and lets torch.autograd differentiate: parameter gradients summed over the views, camera
tensors as leaves, one means2D probe per view.  No derivative is written by hand.  The thresholds are the float32 constants the kernels
compare against (0.2f, 1.3f * tanfov, 0.3f, 0.1f, 1e-7f), so that a value placed ON a threshold is on it in the reference too.

CASES.  One seeded builder per case (`CASES`, `case(name)`).  Every visible Gaussian carries the loss at one to three pixels, chosen on
the float64 projection so that every Gaussian's alpha there is within [2/255, 0.495] or below 0.5/255 and at most six overlap (T >=
0.5^6): no alpha, saturation or transmittance test can flip between float32 and float64.  A decision compared exactly is either exact
in float32 (identity rotation, power-of-two depth: listed in `Case.exact`) or further than MARGIN_REL from its threshold
(`ambiguous()`).  det = a c - b b returns the roundings of a, b and c (a c + b b) / det-fold, while the floor below counts every
rounding once: a case keeps that factor at or below KAPPA_MAX = 4, the margin (`ill_conditioned()`; a Gaussian of 1 : 1 : 100 lies along
an image axis at full length, and 30 degrees off it only as long as the 0.3 dilation leaves its footprint within 8 : 1).  Loss weights,
colours and the background are positive, so the colour dot product of the compositing backward does not cancel: what the bounds
measure is the projection.

BOUNDS.  Decisions (cull, radius, tile count, num_rendered) are exact.  A float record or a gradient row may deviate by
max(4 * E_oracle, n * 2^-24) of the row's own largest reference element (`bound()`); E_oracle is the float32 CPU oracle's deviation on
the same case and output.  n counts the rounded operations on the longest dependent chain of the code, a fused multiply-add as one:
    view depth tz: mul, fma, fma, add                                                                     4    N["tz"]
    pixel centre: hw (4), + 1e-7, reciprocal, * hx, + 1, * W, - 1 (the halving is exact)                  10   N["pix"]
    tx / tz, clamp * tz, focal * tx, * 1 / tz^2  (J02)                                              4 +   4 =  8
    A = J00 V + J02 V (2), Sigma3 A^T (3), a = A Sigma3 A^T + 0.3 (4), det = a c - b b (2)                +11 = 19
    conic = c * (1 / det)                                                                                 +2 = 21   N["conic"]
    d2 = 1 / (det det) (2), dL/db = (2bc gA - (det + 2bb) gB + 2ab gC) d2 (5 behind det)                  19 + 5 = 24
    G2 A (2), Sigma3 gradient A^T G2 A (2), its sum over the views (1)                                    +5 = 29   (dL/dcov3D)
    2 (G3 R) s: three terms and the scale (4), dR = . s (1), the eight products of a quaternion entry (8) +13 = 42
    in front of the chain: gA = -0.5 o g (2) from a moment that is a float32 sum of one to three pixels (3)  +5 = 47
n = 48 for every gradient row (N_GRAD) and, per entry relative to the tensor's largest, for the camera tensors: the additions of their
block reduction are not counted.  pix is measured against the frame's larger side, the scale of (ndc + 1) W.
ONE case, `long thin off-axis`, is held to kappa * n * 2^-24 in place of the floor on the gradients chained through dL/dcov2D (Case.kappa_scaled, `case_kappa()`,
THROUGH_DET; 4 E_oracle as everywhere): its footprints of 13 : 1, turned 30 and 60 degrees off the image axes, are what trained scenes are full of and
what the cap of CASES excludes from every other case; kappa = (a c + b b) / det is the factor by which det returns the roundings of
its inputs.  This is a deviation from the floor the other cases share, made so that such footprints are bounded by a test at all.
The factor four has the standing of the loss suite's: the device's backward is compiled with contraction on and sums its moments in
float32, both of the oracle's own order.  The oracle itself is held to `oracle_bound`: the floor, plus for a gradient the first-order
effect of its own float32 records (`sensitivity()`), from which it differentiates in float64.
"""
import math
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

from splatloc_amd.camera import PinholeCamera
from tests.torch_dense_ref import C0, TILE, quat_to_rot, render_dense

F32 = np.float32
D = torch.float64
NEAR_Z = float(F32(0.2))
DILATION = float(F32(0.3))
DISC_FLOOR = float(F32(0.1))
PW_EPS = float(F32(0.0000001))
MARGIN = 4.0
MARGIN_REL = 1e-4
U = 2.0 ** -24
N = dict(tz=4, pix=10, conic=21)
N_GRAD = 48
KAPPA_MAX = MARGIN
THROUGH_DET = ("m3", "sca", "rot", "cov", "scaling", "rotation", "view")     # gradients chained through dL/dcov2D
ALPHA_LO, ALPHA_HI, ALPHA_DEAD, MAX_OVERLAP = 2.0 / 255.0, 0.495, 0.5 / 255.0, 6

FORWARD_MODELS = ("cull_ge", "no_dilation_c", "no_floor", "radius_small_eig", "rect_no_roundup", "rect_unclamped", "quat_normalised",
                  "no_pw_eps")
GATE_MODELS = ("gate_missing", "gate_on_tz", "gate_one_side")
GRAD_MODELS = ("dcov_no_factor2", "dscale_no_modifier", "m2_pixel_units", "window_last_sigma")
MODELS = FORWARD_MODELS + GATE_MODELS + GRAD_MODELS
MODEL_TEXT = dict(
    cull_ge="cull with >=", gate_missing="gate missing", gate_on_tz="gate also on the tz terms of J02 / J12",
    gate_one_side="gate taken from the positive side only", no_dilation_c="dilation missing on c", no_floor="no 0.1 floor",
    radius_small_eig="radius from the smaller eigenvalue", rect_no_roundup="rectangle without the TILE - 1 round-up",
    rect_unclamped="rectangle unclamped at gx", quat_normalised="quaternion normalised in the plain path",
    dcov_no_factor2="factor 2 on the off-diagonal dcov missing", dscale_no_modifier="scale_modifier missing from dscale",
    no_pw_eps="1e-7 missing from p_w", m2_pixel_units="means2D gradient in pixel units", window_last_sigma="window keeps the last view's dL/dSigma3")


# =================================================================================================================================
# the projection of one view, float64
# =================================================================================================================================
def _sat(v):
    """f2i_sat of preprocess.hip: NaN and everything below -1e9 become -1e9, everything above 1e9 becomes 1e9, then truncation"""
    v = torch.where(v > -1.0e9, v, torch.full_like(v, -1.0e9))
    v = torch.where(v < 1.0e9, v, torch.full_like(v, 1.0e9))
    return torch.trunc(v)


def f32_focal(n, tanfov):
    return float(F32(n) / (F32(2.0) * F32(tanfov)))


def f32_limit(tanfov):
    return float(F32(1.3) * F32(tanfov))


def project(H, W, tanfovx, tanfovy, means3D, Sigma, Vm, PMm, probe=None, model=frozenset()):
    """Gaussians [P,3] with 3D covariance Sigma [P,3,3] under the row-vector view matrix Vm and view-projection matrix PMm.
    Returns the dict render_dense takes as `projection`, plus r3 = 3 sqrt(lambda), the clamp flags cx / cy, txtz / tytz, tiles
    and disc2 = mid^2 - det.  `model`: names of MODELS (the forward and gate ones are applied here)."""
    P = means3D.shape[0]
    hom = torch.cat([means3D, torch.ones(P, 1, dtype=D)], dim=1)
    pv, ph = hom @ Vm, hom @ PMm
    tz = pv[:, 2]
    in_front = (tz >= NEAR_Z) if "cull_ge" in model else (tz > NEAR_Z)
    pw = 1.0 / (ph[:, 3] + (0.0 if "no_pw_eps" in model else PW_EPS))
    ndc = ph[:, :2] * pw[:, None]
    if probe is not None:
        ndc = ndc + probe
    fx, fy = f32_focal(W, tanfovx), f32_focal(H, tanfovy)

    def clamped(t0, lim):
        r = t0 / tz
        over_p, over_n = r > lim, r < -lim
        fwd = torch.minimum(torch.full_like(r, lim), torch.maximum(torch.full_like(r, -lim), r)) * tz   # fminf(lim, fmaxf(-lim, r)) tz
        through = t0 + (fwd - t0).detach()          # the forward's value with the unclamped derivative
        if "gate_missing" in model:
            t = torch.where(over_p | over_n, through, t0)
        elif "gate_one_side" in model:
            t = torch.where(over_p, fwd.detach(), torch.where(over_n, through, t0))
        else:                                       # the lineage: a clamped t.x / t.y is a constant, t.z stays live in J
            t = torch.where(over_p | over_n, fwd.detach(), t0)
        return t, over_p | over_n, r

    tx, cx_, txtz = clamped(pv[:, 0], f32_limit(tanfovx))
    ty, cy_, tytz = clamped(pv[:, 1], f32_limit(tanfovy))
    J02, J12 = -(fx * tx) / (tz * tz), -(fy * ty) / (tz * tz)
    if "gate_on_tz" in model:
        J02, J12 = torch.where(cx_, J02.detach(), J02), torch.where(cy_, J12.detach(), J12)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, J02, zero, fy / tz, J12], dim=1).view(P, 2, 3)
    A = J @ Vm[:3, :3].transpose(0, 1)
    cov2 = A @ Sigma @ A.transpose(1, 2)
    a = cov2[:, 0, 0] + DILATION
    b = cov2[:, 0, 1]
    c = cov2[:, 1, 1] + (0.0 if "no_dilation_c" in model else DILATION)
    det = a * c - b * b
    ok = in_front & (det != 0)
    det_s = torch.where(det != 0, det, torch.ones_like(det))
    mid = 0.5 * (a + c)
    disc2 = mid * mid - det
    disc = torch.sqrt(torch.clamp_min(disc2, 0.0 if "no_floor" in model else DISC_FLOOR))
    r3 = 3.0 * torch.sqrt((mid - disc) if "radius_small_eig" in model else torch.maximum(mid + disc, mid - disc))
    radius = _sat(torch.ceil(r3)).detach()
    pix = torch.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], dim=1)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    pd = pix.detach()
    up = 0.0 if "rect_no_roundup" in model else float(TILE - 1)
    hi_x, hi_y = (1.0e9, 1.0e9) if "rect_unclamped" in model else (gx, gy)
    rminx = _sat((pd[:, 0] - radius) / TILE).clamp(0, gx)
    rminy = _sat((pd[:, 1] - radius) / TILE).clamp(0, gy)
    rmaxx = _sat((pd[:, 0] + radius + up) / TILE).clamp(0, hi_x)
    rmaxy = _sat((pd[:, 1] + radius + up) / TILE).clamp(0, hi_y)
    tiles = (rmaxx - rminx) * (rmaxy - rminy)
    ok = ok & (tiles > 0)
    return dict(tz=tz, ok=ok, con_a=c / det_s, con_b=-b / det_s, con_c=a / det_s, pix=pix, rminx=rminx, rminy=rminy, rmaxx=rmaxx,
                rmaxy=rmaxy, radii=torch.where(ok, radius, torch.zeros_like(radius)).to(torch.int64),
                tiles=torch.where(ok, tiles, torch.zeros_like(tiles)).to(torch.int64), r3=r3, cx=cx_, cy=cy_, txtz=txtz, tytz=tytz,
                disc2=disc2, in_front=in_front)


# =================================================================================================================================
# cases
# =================================================================================================================================
@dataclass
class Case:
    name: str
    W: int
    H: int
    tanfovx: float
    tanfovy: float
    views: list                                   # per view (viewmatrix [4,4], projmatrix [4,4], campos [3]) float32
    means3D: np.ndarray
    opacities: np.ndarray = None                  # [P,1]; None with raw parameters
    colors: np.ndarray = None                     # [P,C] precomputed colours, or
    shs: np.ndarray = None                        # [P,M,3] with sh_degree (single view)
    sh_degree: int = 0
    scales: np.ndarray = None
    rotations: np.ndarray = None
    cov: np.ndarray = None                        # [P,6] precomputed covariance instead of scales / rotations
    raw: tuple = None                             # (scaling [P,3], rotation [P,4], opacity [P,1], f_dc [P,1,3], extra [P,E] or None)
    mod: float = 1.0
    bg: np.ndarray = None
    models: tuple = ()                            # the wrong models this case must expose
    exact: frozenset = frozenset()                # (quantity, view, Gaussian) decided exactly in float32
    forward_only: bool = False
    kappa_scaled: bool = False                    # the floor of its gradients is kappa-fold (module docstring, BOUNDS)
    edge: object = None                           # predicate(reference) -> count proving the case reaches its edge
    pixels: list = field(default_factory=list)    # per view [(y, x, Gaussian)]
    grads: list = field(default_factory=list)     # per view (dL/dcolor [C,H,W], dL/ddepth [1,H,W], dL/dalpha [1,H,W]) float32

    @property
    def P(self):
        return self.means3D.shape[0]

    @property
    def V(self):
        return len(self.views)

    @property
    def C(self):
        if self.raw is not None:
            return 3 + (0 if self.raw[4] is None else self.raw[4].shape[1])
        return 3 if self.shs is not None else self.colors.shape[1]


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def _camera(W, H, fx, fy, R=None, t=None):
    cam = PinholeCamera(W, H, fx, fy, W / 2.0, H / 2.0, None if R is None else torch.tensor(R, dtype=torch.float32),
                        None if t is None else torch.tensor(t, dtype=torch.float32))
    return cam, (cam.world_view_transform.numpy().astype(F32), cam.full_proj_transform.numpy().astype(F32),
                 cam.camera_center.numpy().astype(F32))


def _rot_y(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def _rot_x(a):
    return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])


def _world(view, pts):
    """world positions of the view-space points pts [n,3] under the row-vector view matrix"""
    Vm = view[0].astype(np.float64)
    return ((np.asarray(pts, np.float64) - Vm[3, :3]) @ np.linalg.inv(Vm[:3, :3])).astype(F32)


def _colors(rs, P, C):
    return (0.5 + 0.5 * rs.rand(P, C)).astype(F32)


def _sigma_of(case, scales, rotations, cov, model=frozenset()):
    if cov is not None:
        c = cov
        return torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], dim=1).view(-1, 3, 3)
    if "quat_normalised" in model:
        rotations = rotations / rotations.norm(dim=1, keepdim=True)
    L = quat_to_rot(rotations) * (case.mod * scales)[:, None, :]
    return L @ L.transpose(1, 2)


def _t64(a, grad=False):
    return None if a is None else torch.tensor(np.asarray(a, np.float64), dtype=D, requires_grad=grad)


def _activate(raw):
    """exp / normalize / sigmoid / degree-0 SH + clamp + [rgb | extra] of torch tensors"""
    sc_r, ro_r, op_r, fd_r, ex_r = raw
    rgb = torch.clamp_min(C0 * fd_r[:, 0, :] + 0.5, 0.0)
    return (torch.exp(sc_r), ro_r / ro_r.norm(dim=1, keepdim=True), torch.sigmoid(op_r),
            rgb if ex_r is None else torch.cat([rgb, ex_r], dim=1))


def plain_inputs(case):
    """(opacities, colors, scales, rotations) float32 of a case — of a raw case: the activations in float32 numpy"""
    if case.raw is None:
        return case.opacities, case.colors, case.scales, case.rotations
    from oracle import activations as OA
    sc_r, ro_r, op_r, fd_r, ex_r = case.raw
    with np.errstate(invalid="ignore"):             # (the view direction of a NaN mean: not read at degree 0)
        a = OA.forward(case.means3D, fd_r, np.zeros((case.P, 0, 3), F32), sc_r, ro_r, op_r, ex_r, np.zeros(3, F32), 0)
    return a["opacities"], a["colors"], a["scales"], a["rotations"]


def _finite_rows(case):
    return np.isfinite(case.means3D).all(axis=1)


def _projections(case, model=frozenset()):
    """no-grad projection of every view on the case's own values"""
    with torch.no_grad():
        if case.raw is not None:
            sca, rot, _, _ = _activate([_t64(a) for a in case.raw])
            Sigma = _sigma_of(case, sca, rot, None)
        else:
            Sigma = _sigma_of(case, _t64(case.scales), _t64(case.rotations), _t64(case.cov), model)
        return [project(case.H, case.W, case.tanfovx, case.tanfovy, _t64(case.means3D), Sigma, _t64(v[0]), _t64(v[1]), model=model)
                for v in case.views]


def _light(case, rs, npix=2):
    """Chooses the loss pixels of every view and writes the output gradients (module docstring, CASES)."""
    H, W, P = case.H, case.W, case.P
    opa = plain_inputs(case)[0].reshape(-1).astype(np.float64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    case.pixels, case.grads = [], []
    for pr in _projections(case):
        ok = pr["ok"].numpy()
        vis = np.nonzero(ok)[0]
        alpha = np.zeros((P, H, W))
        for i in vis:
            px, py = pr["pix"][i].numpy()
            dx, dy = px - xs, py - ys
            power = -0.5 * (float(pr["con_a"][i]) * dx * dx + float(pr["con_c"][i]) * dy * dy) - float(pr["con_b"][i]) * dx * dy
            inr = ((xs // TILE >= float(pr["rminx"][i])) & (xs // TILE < float(pr["rmaxx"][i]))
                   & (ys // TILE >= float(pr["rminy"][i])) & (ys // TILE < float(pr["rmaxy"][i])))
            assert (power[inr] <= -1e-9).all() or (power <= 0).all()
            alpha[i] = np.where(inr, opa[i] * np.exp(np.minimum(power, 0.0)), 0.0)
        band = (alpha >= ALPHA_LO) & (alpha <= ALPHA_HI)
        dead = alpha < ALPHA_DEAD
        clean = (band | dead).all(axis=0) & (band.sum(axis=0) <= MAX_OVERLAP)
        taken = np.zeros((H, W), bool)
        pix = []
        for i in vis:
            # alone on the pixel first; then at least one deviation from the centre (alpha <= e^-1/2 of the opacity), where the gradient
            # of the centre is largest and least sensitive to the float32 rounding of the centre itself; then the brightest
            score = np.where(band[i] & clean & ~taken, alpha[i] + 10.0 * (band.sum(axis=0) == 1) + 5.0 * (alpha[i] <= 0.6065 * opa[i]), -1.0)
            for _ in range(npix):
                y, x = np.unravel_index(int(np.argmax(score)), score.shape)
                if score[y, x] < 0:
                    break
                pix.append((int(y), int(x), int(i)))
                taken[y, x] = True
                score[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = -1.0      # (the next one not adjacent: another offset from the centre)
                # ... and in the same quadrant about the centre: pixels on opposite sides cancel in dL/dmeans2D, and a row that is
                # the small difference of two terms has no meaningful maximum of its own
                cpx, cpy = pr["pix"][i].numpy()
                score[((xs - cpx) * (x - cpx) < 0) | ((ys - cpy) * (y - cpy) < 0)] = -1.0
            assert any(p[2] == i for p in pix), f"{case.name}: Gaussian {i} reaches no usable pixel"
        gc, gd, ga = np.zeros((case.C, H, W), F32), np.zeros((1, H, W), F32), np.zeros((1, H, W), F32)
        for y, x, _ in pix:
            gc[:, y, x] = 0.5 + rs.rand(case.C)
            gd[0, y, x] = 0.25 + 0.5 * rs.rand()
            ga[0, y, x] = 0.5 + rs.rand()
        case.pixels.append(pix)
        case.grads.append((gc, gd, ga))
    return case


def ambiguous(case):
    """(quantity, view, Gaussian) of every decision closer than MARGIN_REL to its threshold and not listed in case.exact"""
    out = []
    gx, gy = (case.W + TILE - 1) // TILE, (case.H + TILE - 1) // TILE
    fin = _finite_rows(case)
    for v, pr in enumerate(_projections(case)):
        def near(q, thr):
            return abs(q - thr) <= MARGIN_REL * abs(thr)
        for i in range(case.P):
            if not fin[i] or not math.isfinite(float(pr["r3"][i])):
                continue
            bad = []
            if near(float(pr["tz"][i]), NEAR_Z):
                bad.append("tz")
            if not bool(pr["in_front"][i]):
                out += [(q, v, i) for q in bad if (q, v, i) not in case.exact]
                continue
            for q, lim in (("txtz", f32_limit(case.tanfovx)), ("tytz", f32_limit(case.tanfovy))):
                if near(abs(float(pr[q][i])), lim):
                    bad.append(q)
            r3 = float(pr["r3"][i])
            if near(r3, round(r3)):
                bad.append("radius")
            if near(float(pr["disc2"][i]), DISC_FLOOR):
                bad.append("floor")
            rad = math.ceil(r3)
            px, py = (float(t) for t in pr["pix"][i])
            for q, g in (((px - rad) / TILE, gx), ((py - rad) / TILE, gy), ((px + rad + TILE - 1) / TILE, gx), ((py + rad + TILE - 1) / TILE, gy)):
                k = round(q)
                if 1 <= k <= g and near(q, k):
                    bad.append("rect")
            out += [(q, v, i) for q in bad if (q, v, i) not in case.exact]
    return out


def _kappas(case):
    """(view, Gaussian, (a c + b b) / det) of every visible row"""
    out = []
    for v, pr in enumerate(_projections(case)):
        A, B, C = (pr[k].numpy() for k in ("con_a", "con_b", "con_c"))      # (the conic's factor is the covariance's)
        with np.errstate(invalid="ignore", divide="ignore"):
            kappa = (A * C + B * B) / (A * C - B * B)
        out += [(v, int(i), float(kappa[i])) for i in np.nonzero(pr["ok"].numpy())[0]]
    return out


def ill_conditioned(case):
    """(view, Gaussian, factor) of every visible row whose determinant amplifies the roundings of a, b, c more than KAPPA_MAX-fold
    (none by definition in the case whose floor is scaled by that factor)"""
    return [] if case.kappa_scaled else [k for k in _kappas(case) if not k[2] <= KAPPA_MAX]


_KAPPA = {}


def case_kappa(case):
    if case.name not in _KAPPA:
        _KAPPA[case.name] = max(k[2] for k in _kappas(case))
    return _KAPPA[case.name]


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
IDQ = (1.0, 0.0, 0.0, 0.0)


def _layout(name, W, H, fx, fy, rows, R=None, t=None, **kw):
    """rows: (txtz, tytz, tz, sigma_x px, sigma_y px, scale z, quaternion, opacity) per Gaussian, placed in VIEW space: sigma is the
    screen-space deviation an axis-aligned Gaussian of that depth gets on the optical axis"""
    cam, view = _camera(W, H, fx, fy, R, t)
    rows = [tuple(r) + (IDQ, 0.4)[len(r) - 6:] for r in rows]
    pts = np.array([[F32(r[0]) * F32(r[2]), F32(r[1]) * F32(r[2]), F32(r[2])] for r in rows], F32)
    mod = kw.get("mod", 1.0)
    scales = np.array([[r[3] * abs(r[2]) / fx / mod, r[4] * abs(r[2]) / fy / mod, r[5] / mod] for r in rows], F32)
    means = pts if R is None and t is None else _world(view, pts)
    return Case(name=name, W=W, H=H, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, views=[view], means3D=means,
                opacities=np.array([[r[7]] for r in rows], F32), scales=scales, rotations=np.array([r[6] for r in rows], F32),
                bg=np.full((3,), 0.25, F32), **kw)


def _cov_of(case):
    """the case with its covariance precomputed (float32 of the float64 product)"""
    with torch.no_grad():
        S = _sigma_of(case, _t64(case.scales), _t64(case.rotations), None).numpy()
    case.cov = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1).astype(F32)
    case.scales = case.rotations = None
    case.mod = 1.0
    return case


def _to_raw(case, rs, E):
    """the case through the raw parameters: log / unnormalised quaternion / logit / degree-0 SH coefficient (+ E extra channels)"""
    q = case.rotations.astype(np.float64) * (0.5 + rs.rand(case.P, 1))
    op = case.opacities.astype(np.float64)
    rgb = 0.5 + 0.5 * rs.rand(case.P, 3)
    case.raw = (np.log(case.scales.astype(np.float64)).astype(F32), q.astype(F32), np.log(op / (1 - op)).astype(F32),
                ((rgb - 0.5) / C0).astype(F32).reshape(case.P, 1, 3), (0.5 + 0.5 * rs.rand(case.P, E)).astype(F32) if E else None)
    case.opacities = case.colors = case.scales = case.rotations = None
    return case


LIM = float(F32(1.3))                     # 1.3f * tanfov at tanfov = 1
LIM_UP = float(np.nextafter(F32(1.3), F32(2)))
NEAR_UP = float(np.nextafter(F32(0.2), F32(1)))


def _count_clamped(ref):
    """visible-and-clamped (view, Gaussian) rows whose Gaussian carries a non-zero gradient"""
    live = np.abs(ref["m3"]).max(axis=1) > 0
    return int(((ref["cx"] | ref["cy"]) & ref["ok"] & live[None]).sum())


def _count_near_plane(ref):
    """Gaussians within 2 ulps of the cull plane: (at or below it, above it)"""
    tz = ref["tz_all"].astype(F32)
    d = np.abs(tz.view(np.int32).astype(np.int64) - int(F32(0.2).view(np.int32)))
    return int(((d <= 2) & (tz <= F32(0.2))).sum()), int(((d <= 2) & (tz > F32(0.2))).sum())


def _cull(name, raw=None):
    rs = _rs(name)
    # identity view: tz IS means3D.z.  sigma 2 px; spread over the frame
    zs = [NEAR_Z, NEAR_UP, 0.25, 0.5, -1.0, float("nan"), 1.0]
    at = [(-0.6, -0.5), (0.0, -0.5), (0.6, -0.5), (-0.6, 0.5), (0.0, 0.5), (0.6, 0.5), (0.0, 0.0)]
    c = _layout(name, 48, 32, 24.0, 16.0, [(x, y, z, 2.0, 2.0, 0.01 * (abs(z) if z == z else 1.0)) for (x, y), z in zip(at, zs)],
                models=("cull_ge",), exact=frozenset(("tz", 0, i) for i in (0, 1)),
                edge=lambda ref: min(_count_near_plane(ref)))
    c.means3D[5] = (0.3, 0.25, np.nan)
    c.scales[5] = (0.02, 0.02, 0.01)
    c.colors = _colors(rs, c.P, 4)
    if raw is not None:
        _to_raw(c, rs, raw)
    return _light(c, rs)


def _clamp_rows(axis):
    vals = [1.2, LIM, LIM_UP, 1.4, 1.6]
    rows = []
    for sgn in (1.0, -1.0):
        for k, u in enumerate(vals):
            w = (k - 2) * 0.35
            rows.append((sgn * u, w, 2.0, 8.0, 2.0, 0.05) if axis == 0 else (w, sgn * u, 2.0, 2.0, 6.0, 0.05))
    return rows


def _clamp_x(name, raw=None):
    rs = _rs(name)
    c = _layout(name, 48, 32, 24.0, 16.0, _clamp_rows(0), models=GATE_MODELS + ("m2_pixel_units",),
                exact=frozenset(("txtz", 0, i) for i in (1, 2, 6, 7)), edge=_count_clamped)
    c.colors = _colors(rs, c.P, 4)
    if raw is not None:
        _to_raw(c, rs, raw)
    return _light(c, rs)


def _clamp_y(name):
    rs = _rs(name)
    c = _layout(name, 48, 32, 24.0, 16.0, _clamp_rows(1), models=GATE_MODELS + ("dcov_no_factor2",),
                exact=frozenset(("tytz", 0, i) for i in (1, 2, 6, 7)), edge=_count_clamped)
    c.colors = _colors(rs, c.P, 4)
    # a z rotation of a few degrees: off-diagonal covariance entries for dcov
    a = 0.1
    c.rotations[:] = (math.cos(a / 2), 0.0, 0.0, math.sin(a / 2))
    return _light(_cov_of(c), rs)


def _clamp_xy(name):
    rs = _rs(name)
    # rotated and translated camera (dense view matrix), scale_modifier 1.6: one Gaussian clamped in both, one in x, one in y, two free
    rows = [(1.5, 1.5, 2.0, 8.0, 8.0, 0.05), (-1.45, 0.3, 2.0, 8.0, 1.5, 0.05), (0.2, -1.5, 2.5, 1.5, 7.0, 0.05),
            (0.1, 0.45, 2.0, 2.0, 2.0, 0.05), (-0.3, -0.2, 3.0, 2.5, 1.5, 0.2, (0.9, 0.1, -0.3, 0.2))]
    c = _layout(name, 48, 32, 24.0, 16.0, rows, R=_rot_y(0.2) @ _rot_x(-0.1), t=(0.1, -0.05, 0.4), mod=1.6,
                models=GATE_MODELS + ("dscale_no_modifier",), edge=_count_clamped)
    c.colors = _colors(rs, c.P, 4)
    return _light(c, rs)


def _solve_sigma(W, H, fx, fy, row, target):
    """the screen deviation (both axes) at which the Gaussian `row` has 3 sqrt(lambda) = target: bisection on the float64 projection"""
    lo, hi = 0.05, 40.0
    for _ in range(80):
        s = 0.5 * (lo + hi)
        c = _layout("solve", W, H, fx, fy, [row[:3] + (s, s, row[5])])
        r3 = float(_projections(c)[0]["r3"][0])
        lo, hi = (s, hi) if r3 < target else (lo, s)
    return 0.5 * (lo + hi)


def _conic(name):
    rs = _rs(name)
    W, H, fx, fy = 48, 32, 24.0, 16.0
    q_long_x = (math.sqrt(0.5), 0.0, math.sqrt(0.5), 0.0)                       # the long (z) scale axis turned into view x
    az = math.radians(30.0)
    q_z = np.array([math.cos(az / 2), 0, 0, math.sin(az / 2)])
    q_long_30 = _qmul(q_z, np.array(q_long_x))                                  # ... and then 30 degrees in the image plane
    below = _solve_sigma(W, H, fx, fy, (0.65, -0.5, 2.0, 0, 0, 0.02), 4.0 - 0.0007)
    above = _solve_sigma(W, H, fx, fy, (0.65, 0.5, 2.0, 0, 0, 0.02), 4.0 + 0.0007)
    rows = [(-0.7, -0.5, 2.0, 2.5, 2.5, 2.5 * 2.0 / 24.0),                       # isotropic
            (-0.25, -0.5, 2.0, 0.05, 0.05 * 16.0 / 24.0, 100 * 0.05 * 2.0 / 24.0, q_long_x),    # 1 : 1 : 100 along the image x axis
            (0.2, -0.5, 2.0, 0.015, 0.015 * 16.0 / 24.0, 100 * 0.015 * 2.0 / 24.0, tuple(q_long_30)),    # the same, short enough for KAPPA_MAX
            (-0.7, 0.5, 1.0, 0.002, 0.002, 0.0001),                               # only the dilation remains: the floor, radius 3
            (-0.3, 0.5, 2.0, 3.0, 1.5, 0.1, (0.9 * 1.3, 0.2 * 1.3, -0.3 * 1.3, 0.25 * 1.3)),   # |q| = 1.3 * 0.995: used as passed
            (0.2, 0.5, 2.0, 3.0, 1.5, 0.1, tuple(np.array((0.9, 0.2, -0.3, 0.25)) / math.sqrt(0.9925))),   # the unit one
            (0.65, -0.5, 2.0, below, below, 0.02), (0.65, 0.5, 2.0, above, above, 0.02)]
    c = _layout(name, W, H, fx, fy, rows, models=("no_dilation_c", "no_floor", "radius_small_eig", "quat_normalised"),
                edge=lambda ref: int((ref["disc2"][0, 3] < DISC_FLOOR) and ref["radii"][0, 3] == 3 and ref["radii"][0, 6] == 4
                                     and ref["radii"][0, 7] == 5 and 4e-4 < 4 - ref["r3"][0, 6] < 1e-3 and 4e-4 < ref["r3"][0, 7] - 4 < 1e-3))
    c.colors = _colors(rs, c.P, 4)
    return _light(c, rs)


def _long_thin(name):
    """1 : 1 : 100 Gaussians whose footprints lie 30 and 60 degrees off the image x axis at 4 px by 0.55 px, one along it"""
    rs = _rs(name)
    q_long_x = np.array((math.sqrt(0.5), 0.0, math.sqrt(0.5), 0.0))
    qz = lambda deg: np.array([math.cos(math.radians(deg) / 2), 0, 0, math.sin(math.radians(deg) / 2)])  # noqa: E731
    row = lambda x, y, s, q: (x, y, 2.0, s, s * 16.0 / 24.0, 100 * s * 2.0 / 24.0, tuple(q))  # noqa: E731
    rows = [row(-0.5, -0.4, 0.04, _qmul(qz(30.0), q_long_x)), row(0.4, 0.3, 0.04, _qmul(qz(60.0), q_long_x)), row(-0.4, 0.5, 0.04, q_long_x)]
    c = _layout(name, 48, 32, 24.0, 16.0, rows, models=("no_dilation_c", "radius_small_eig", "gate_missing"), kappa_scaled=True,
                edge=lambda ref: int(case_kappa(case(name)) > 2 * KAPPA_MAX))
    c.colors = _colors(rs, c.P, 4)
    return _light(c, rs)


def _qmul(a, b):
    r1, x1, y1, z1 = a
    r2, x2, y2, z2 = b
    return np.array([r1 * r2 - x1 * x2 - y1 * y2 - z1 * z2, r1 * x2 + x1 * r2 + y1 * z2 - z1 * y2,
                     r1 * y2 - x1 * z2 + y1 * r2 + z1 * x2, r1 * z2 + x1 * y2 - y1 * x2 + z1 * r2])


def _ndc_of(pix, n):
    return (2.0 * pix + 1.0) / n - 1.0


def _rect(name):
    rs = _rs(name)
    W = H = 33
    f = 16.5
    r16 = _solve_sigma(W, H, f, f, (0.0, 0.0, 2.0, 0, 0, 0.02), 15.5)            # radius 16 on the centre pixel 16.0: rmin = 0 exactly
    rall = _solve_sigma(W, H, f, f, (0.0, 0.0, 4.0, 0, 0, 0.02), 33.5)           # radius 34: every tile
    n = lambda p: _ndc_of(p, 33)  # noqa: E731
    rows = [(0.0, 0.0, 2.0, r16, r16, 0.02, IDQ, 0.3), (0.0, 0.0, 4.0, rall, rall, 0.02, IDQ, 0.2),
            (n(1.0), n(7.0), 1.0, 1.2, 1.2, 0.01), (n(31.5), n(24.0), 1.0, 1.2, 1.2, 0.01),     # over the left and the right edge
            (n(24.0), n(0.5), 1.0, 1.2, 1.2, 0.01), (n(8.0), n(32.0), 1.0, 1.2, 1.2, 0.01),     # over the top and the bottom edge
            (n(32.0), n(32.0), 1.5, 1.2, 1.2, 0.01),                                             # over the corner
            (n(-3.0), n(26.0), 1.0, 1.6, 1.6, 0.01),                                             # centre outside, rectangle inside
            (n(-20.0), n(16.0), 1.0, 1.2, 1.2, 0.01)]                                            # zero area: culled
    c = _layout(name, W, H, f, f, rows, models=("rect_no_roundup", "rect_unclamped"), exact=frozenset({("rect", 0, 0)}),
                edge=lambda ref: int(ref["radii"][0, 0] == 16 and ref["pix"][0, 0, 0] == 16.0 and ref["tiles"][0, 1] == 9
                                     and not ref["ok"][0, 8] and ref["in_front"][0, 8] and ref["ok"][0, 7] and ref["pix"][0, 7, 0] < 0))
    c.colors = _colors(rs, c.P, 4)
    return _light(c, rs)


def _rect_ragged(name):
    rs = _rs(name)
    W, H = 40, 24                                                                 # two and a half by one and a half tiles
    nx, ny = (lambda p: _ndc_of(p, 40)), (lambda p: _ndc_of(p, 24))
    rall = _solve_sigma(W, H, 20.0, 12.0, (0.0, 0.0, 4.0, 0, 0, 0.02), 40.5)
    rows = [(0.0, 0.0, 4.0, rall, rall, 0.02, IDQ, 0.2), (nx(36.5), ny(5.0), 1.0, 1.2, 1.2, 0.01), (nx(10.0), ny(22.0), 1.0, 1.2, 1.2, 0.01),
            (nx(38.5), ny(22.5), 1.5, 1.2, 1.2, 0.01), (nx(20.0), ny(10.0), 1.0, 1.2, 1.2, 0.01), (nx(45.0), ny(12.0), 1.0, 2.5, 2.5, 0.01)]
    c = _layout(name, W, H, 20.0, 12.0, rows, models=("rect_unclamped", "rect_no_roundup"),
                edge=lambda ref: int(ref["tiles"][0, 0] == 6 and ref["ok"][0, 1:].all() and ref["pix"][0, 5, 0] > 40))
    c.colors = _colors(rs, c.P, 4)
    return _light(c, rs)


def _block(name, P):
    rs = _rs(name)
    # P - 1 Gaussians behind the camera but for one in every 41 (small, on a grid); the last is large and visible, the one before
    # it culled by the near plane
    rows = []
    for i in range(P - 1):
        k = i // 41
        vis = i % 41 == 7 and k < 12
        rows.append(((-0.75 + 0.5 * (k % 4)), (-0.6 + 0.6 * (k // 4)), 1.0 if vis else -1.0 - 0.01 * (i % 7), 1.0, 1.0, 0.01))
    if P > 1:
        rows[-1] = (0.0, 0.0, 0.15, 2.0, 2.0, 0.01)
    rows.append((0.1, 0.3, 3.0, 7.0, 7.0, 0.05, IDQ, 0.15))
    c = _layout(name, 48, 32, 24.0, 16.0, rows, models=("rect_unclamped",),
                edge=lambda ref: int(ref["ok"][0, -1] and (P == 1 or not ref["ok"][0, -2])))
    c.colors = _colors(rs, c.P, 4)
    return _light(c, rs, npix=1)


def _window(name, V, raw=None, C=4):
    rs = _rs(name)
    W, H, fx, fy = 48, 32, 24.0, 16.0
    # Gaussian 0 sits in the world origin: a view's translation IS its view-space position, whatever the view's rotation
    pose = [(_rot_y(0.0), (0.0, 0.0, 2.0)),                                   # 0: visible
            (_rot_y(0.3), (0.1, 0.0, 0.125)),                                 # 1: in front of the near plane (tz = 0.125: exact)
            (_rot_y(0.2) @ _rot_x(0.1), (0.3, -0.2, 2.5)),                    # 2: visible
            (_rot_y(-0.25), (2.9, 0.2, 2.0)),                                 # 3: clamped in x (1.45)
            (_rot_y(0.1), (9.0, 0.0, 2.0)), (_rot_x(0.2), (0.0, -9.0, 2.0)), (_rot_y(-0.1), (-9.0, 1.0, 2.0)),
            (_rot_x(-0.15), (1.0, 9.0, 2.0))][:V]                             # 4..7: off screen, zero-area rectangle
    cams = [_camera(W, H, fx, fy, R, t) for R, t in pose]
    s0 = 8.0 * 2.0 / fx
    means = [(0.0, 0.0, 0.0), (0.0, 60.0, 0.0),                               # 1: seen by no view (the views turn about x by 0.2 at most)
             (-0.9, -0.5, 0.3), (0.8, 0.55, -0.2), (-0.6, 0.6, 0.6), (0.7, -0.6, 0.4), (0.2, 0.75, 0.0)]
    scales = [(s0, 0.1, 0.05), (0.1, 0.1, 0.1)] + [(0.16, 0.12, 0.1)] * 5
    rot = [IDQ, IDQ, (0.9, 0.1, -0.3, 0.2), IDQ, (0.8, -0.2, 0.1, 0.5), IDQ, (0.7, 0.3, 0.3, -0.4)]
    c = Case(name=name, W=W, H=H, tanfovx=cams[0][0].tanfovx, tanfovy=cams[0][0].tanfovy, views=[cv[1] for cv in cams],
             means3D=np.array(means, F32), opacities=np.full((7, 1), 0.4, F32), scales=np.array(scales, F32), rotations=np.array(rot, F32),
             bg=np.full((3,), 0.25, F32), models=("window_last_sigma", "gate_missing") if V > 3 else ("window_last_sigma",),
             exact=frozenset({("tz", 1, 0)}),
             edge=lambda ref: int(ref["ok"][0, 0] and not ref["ok"][1, 0] and not ref["ok"][:, 1].any()
                                  and (V < 3 or ref["ok"][2, 0]) and (V < 4 or (ref["ok"][3, 0] and ref["cx"][3, 0]))
                                  and not ref["ok"][4:, 0].any()))
    c.colors = _colors(rs, c.P, C)
    if raw is not None:
        _to_raw(c, rs, raw)
    return _light(c, rs)


def _generic(name, C=4, sh_degree=None):
    """a rotated camera over a handful of generic Gaussians, one of them clamped: the channel counts and SH colours"""
    rs = _rs(name)
    rows = [(-0.7 + 0.45 * (k % 4) + 0.05 * rs.rand(), -0.5 + 1.0 * (k // 4) + 0.05 * rs.rand(), 1.5 + rs.rand(), 1.5 + rs.rand(), 1.5 + rs.rand(),
             0.05 + 0.1 * rs.rand(), tuple(np.array(IDQ) + 0.3 * (rs.rand(4) - 0.5))) for k in range(8)]
    rows.append((1.45, 0.0, 2.0, 8.0, 1.5, 0.05))
    c = _layout(name, 48, 32, 24.0, 16.0, rows, R=_rot_y(-0.15) @ _rot_x(0.1), t=(-0.1, 0.05, 0.3), models=("gate_missing", "m2_pixel_units"),
                edge=_count_clamped)
    if sh_degree is None:
        c.colors = _colors(rs, c.P, C)
    else:
        c.shs = np.concatenate([1.2 + 0.3 * rs.rand(c.P, 1, 3), 0.3 * (rs.rand(c.P, 15, 3) - 0.5)], axis=1).astype(F32)
        c.sh_degree = sh_degree
    return _light(c, rs)


def _pw(name):
    """a view-projection matrix scaled by 2^-12: the same NDC but for the 1e-7 under p_w, now 1e-7 * 2^12 / tz of it"""
    rs = _rs(name)
    c = _layout(name, 48, 32, 24.0, 16.0, [(-0.5, 0.4, 0.25, 2.0, 2.0, 0.005), (0.6, -0.5, 0.5, 2.0, 2.0, 0.01), (0.1, 0.1, 1.0, 2.0, 2.0, 0.02)],
                models=("no_pw_eps",), edge=lambda ref: int(ref["ok"].all()))
    V0, PM0, cp = c.views[0]
    c.views = [(V0, (PM0 * F32(2.0 ** -12)).astype(F32), cp)]
    c.colors = _colors(rs, c.P, 4)
    return _light(c, rs)


def _nonfinite(name):
    """forward only: a NaN and an infinite mean next to healthy Gaussians (an infinite or NaN scale is NOT here: see the GPU file)"""
    rs = _rs(name)
    rows = [(-0.5, -0.4, 1.0, 2.0, 2.0, 0.02), (0.0, 0.0, 1.0, 2.0, 2.0, 0.02), (0.5, 0.4, 2.0, 2.0, 2.0, 0.02), (0.0, 0.0, 1.0, 2.0, 2.0, 0.02),
            (0.0, 0.0, 1.0, 2.0, 2.0, 0.02), (0.0, 0.0, 1.0, 2.0, 2.0, 0.02), (-0.5, 0.4, 1.5, 2.0, 2.0, 0.02)]
    c = _layout(name, 48, 32, 24.0, 16.0, rows, forward_only=True,
                edge=lambda ref: int(ref["ok"][0, [0, 2, 6]].all() and not ref["ok"][0, [1, 3, 4, 5]].any()))
    c.means3D[1] = (np.nan, 0.0, 1.0)
    c.means3D[3] = (0.0, 0.0, np.inf)
    c.means3D[4] = (-np.inf, 0.0, 1.0)
    c.means3D[5] = (0.0, np.inf, np.nan)
    c.colors = _colors(rs, c.P, 4)
    return c


CASES = {
    "cull": _cull, "clamp x": _clamp_x, "clamp y cov3D": _clamp_y, "clamp xy modifier 1.6": _clamp_xy, "conic and radius": _conic,
    "long thin off-axis": _long_thin, "rect 33x33": _rect, "rect ragged 40x24": _rect_ragged, "p_w epsilon": _pw,
    **{f"block P {P}": (lambda n, P=P: _block(n, P)) for P in (1, 255, 256, 257, 513)},
    **{f"window V {V}": (lambda n, V=V: _window(n, V)) for V in (2, 5, 8)},
    "channels 3": lambda n: _generic(n, 3), "channels 4": lambda n: _generic(n, 4), "channels 35": lambda n: _generic(n, 35),
    "channels 40": lambda n: _generic(n, 40), "sh degree 2": lambda n: _generic(n, sh_degree=2),
    "raw cull E 0": lambda n: _cull(n, raw=0), "raw clamp x E 1": lambda n: _clamp_x(n, raw=1), "raw window V 5 E 1": lambda n: _window(n, 5, raw=1),
    "raw window V 2 E 0": lambda n: _window(n, 2, raw=0),
    "non-finite means": _nonfinite,
}
_BUILT = {}


def case_names(backward=None):
    return [n for n in CASES if backward is None or (n != "non-finite means") == backward]


def case(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name](name)
    return _BUILT[name]


# =================================================================================================================================
# the reference of a case
# =================================================================================================================================
GRADS = ("m3", "op", "col", "sca", "rot", "cov", "sh", "scaling", "rotation", "opacity", "f_dc", "extra")
_REFS = {}


def reference(case, model=frozenset(), perturb=None):
    """Decisions, records and (unless case.forward_only) gradients of a case, numpy float64; cached for the empty model.
    ok / radii / tiles / cx / cy / in_front [V,P], num_rendered [V], pix [V,P,2], tz [V,P] and conic [V,P,3] (zero rows where culled,
    as the device records them), tz_all (unmasked), r3, disc2; gradients GRADS (None when absent), m2 [V,P,2], view / proj [V,4,4],
    campos [V,3]."""
    model = frozenset(model)
    key = case.name
    if not model and perturb is None and key in _REFS:
        return _REFS[key]
    assert model <= set(MODELS)
    prs = _projections(case, model)
    ok = torch.stack([p["ok"] for p in prs]).numpy()
    m = ok[..., None]
    st = lambda k: torch.stack([p[k] for p in prs]).numpy()  # noqa: E731
    out = dict(ok=ok, radii=st("radii"), tiles=st("tiles"), cx=st("cx"), cy=st("cy"), in_front=st("in_front"), tz_all=st("tz"), r3=st("r3"),
               disc2=st("disc2"), num_rendered=st("tiles").sum(axis=1), pix=np.where(m, st("pix"), 0.0), tz=np.where(ok, st("tz"), 0.0),
               conic=np.where(m, np.stack([st("con_a"), st("con_b"), st("con_c")], axis=-1), 0.0))
    if case.forward_only:
        return out
    # rows with a non-finite mean are culled (asserted) and their gradients are zero by definition; autograd sees a finite stand-in
    # behind the camera in their place, because 0 * NaN of the masked branch would spread through the camera leaves
    fin = _finite_rows(case)
    assert not ok[:, ~fin].any() and (fin.all() or all(np.array_equal(v[0], np.eye(4, dtype=F32)) for v in case.views))
    m3 = _t64(np.where(fin[:, None], case.means3D, np.array([0.0, 0.0, -1.0])), True)
    raw = None
    cov = sh = None
    if case.raw is not None:
        raw = [_t64(a, True) for a in case.raw]
        sca, rot, opa, col = _activate(raw)
    else:
        opa, col, sca, rot, cov, sh = (_t64(a, True) for a in (case.opacities, case.colors, case.scales, case.rotations, case.cov, case.shs))
    Sigma = _sigma_of(case, sca, rot, cov, model)
    cams, probes, losses = [], [], []
    for v, (Vn, PMn, cpn) in enumerate(case.views):
        Vm, PMm, cp = _t64(Vn, True), _t64(PMn, True), _t64(cpn, True)
        probe = torch.zeros(case.P, 2, dtype=D, requires_grad=True)
        pr = project(case.H, case.W, case.tanfovx, case.tanfovy, m3, Sigma, Vm, PMm, probe, model)
        assert torch.equal(pr["ok"], prs[v]["ok"])
        if perturb is not None:                     # (sensitivity(): a forward record moved by its own floor)
            rec, comp = perturb
            if rec == "pix":
                shift = torch.zeros(2, dtype=D)
                shift[comp] = floor(case, "pix") * max(case.W, case.H)
                pr["pix"] = pr["pix"] + shift
            elif rec == "tz":
                pr["tz"] = pr["tz"] * (1.0 + floor(case, "tz"))
            else:
                k = ("con_a", "con_b", "con_c")[comp]
                big = torch.stack([pr["con_a"], pr["con_b"], pr["con_c"]]).abs().max(dim=0).values.detach()
                pr[k] = pr[k] + floor(case, "conic") * big
        color, depth, alpha, _ = render_dense(case.H, case.W, case.tanfovx, case.tanfovy, torch.tensor(case.bg), m3, opa, Vm, PMm, cp,
                                              colors_precomp=col, shs=sh, sh_degree=case.sh_degree, projection=pr)
        gc, gd, ga = (_t64(g) for g in case.grads[v])
        losses.append((color * gc).sum() + (depth * gd).sum() + (alpha * ga).sum())
        cams.append((Vm, PMm, cp))
        probes.append(probe)
    named = dict(m3=m3, op=opa, col=col, sca=sca, rot=rot, cov=cov, sh=sh)
    if raw is not None:
        named = dict(m3=m3, scaling=raw[0], rotation=raw[1], opacity=raw[2], f_dc=raw[3], extra=raw[4])
    leaves = [(k, t) for k, t in named.items() if t is not None]
    flat = [t for _, t in leaves] + probes + [t for cam in cams for t in cam]
    g = torch.autograd.grad(sum(losses), flat, allow_unused=True, retain_graph=True)
    zero = lambda t, gr: torch.zeros_like(t) if gr is None else gr  # noqa: E731
    for (k, t), gr in zip(leaves, g):
        out[k] = zero(t, gr).numpy().copy()
    nl = len(leaves)
    out["m2"] = np.stack([zero(probes[v], g[nl + v]).numpy() for v in range(case.V)])
    gc_ = g[nl + case.V:]
    out["view"] = np.stack([zero(cams[v][0], gc_[3 * v]).numpy() for v in range(case.V)])
    out["proj"] = np.stack([zero(cams[v][1], gc_[3 * v + 1]).numpy() for v in range(case.V)])
    out["campos"] = np.stack([zero(cams[v][2], gc_[3 * v + 2]).numpy() for v in range(case.V)])
    for k in GRADS:
        out.setdefault(k, None)
    # ---- the wrong models of the backward ----
    if "window_last_sigma" in model:
        gS = torch.autograd.grad(losses[-1], Sigma, retain_graph=True, allow_unused=True)[0]
        for k in ("sca", "rot", "cov", "scaling", "rotation"):
            if out[k] is not None:
                out[k] = torch.autograd.grad(Sigma, named[k], grad_outputs=gS, retain_graph=True)[0].numpy().copy()
    if "dcov_no_factor2" in model and out["cov"] is not None:
        out["cov"][:, [1, 2, 4]] *= 0.5
    if "dscale_no_modifier" in model and out["sca"] is not None:
        out["sca"] /= case.mod
    if "m2_pixel_units" in model:
        out["m2"] = out["m2"] / np.array([0.5 * case.W, 0.5 * case.H])
    if not model and perturb is None:
        _REFS[key] = out
    return out


# =================================================================================================================================
# the CPU oracle on a case
# =================================================================================================================================
def oracle_run(case):
    """oracle.forward / oracle.backward of every view of a case in the layout of `reference` (parameter gradients summed over the
    views in float64; a raw case through oracle/activations.py), plus rec0 [V,P,4] float32: the device's first record, bit for bit"""
    from oracle import activations as OA
    from oracle import oracle
    opa, col, sca, rot = plain_inputs(case)
    P, V = case.P, case.V
    out = dict(ok=np.zeros((V, P), bool), radii=np.zeros((V, P), np.int64), tiles=np.zeros((V, P), np.int64), num_rendered=np.zeros(V, np.int64),
               pix=np.zeros((V, P, 2)), tz=np.zeros((V, P)), conic=np.zeros((V, P, 3)), rec0=np.zeros((V, P, 4), F32))
    sums = {}
    st = oracle.Settings(case.H, case.W, case.tanfovx, case.tanfovy, scale_modifier=case.mod, sh_degree=case.sh_degree)
    kw = dict(shs=case.shs) if case.shs is not None else dict(colors_precomp=col)
    kw.update(dict(cov3D_precomp=case.cov) if case.cov is not None else dict(scales=sca, rotations=rot))
    m2, cam = [], dict(view=[], proj=[], campos=[])
    for v, (Vn, PMn, cpn) in enumerate(case.views):
        f = oracle.forward(st, case.bg, case.means3D, opa, Vn, PMn, cpn, **kw)
        out["ok"][v], out["radii"][v], out["tiles"][v], out["num_rendered"][v] = f["radii"] > 0, f["radii"], f["tiles_touched"], f["num_rendered"]
        out["pix"][v], out["tz"][v], out["conic"][v] = f["xy"], f["view_depth"], f["conic_opacity"][:, :3]
        out["rec0"][v] = np.concatenate([f["xy"], f["view_depth"][:, None], f["radii"][:, None].astype(F32)], axis=1)
        if case.forward_only:
            continue
        b = oracle.backward(f, *case.grads[v])
        for k, name in (("m3", "dL_dmeans3D"), ("op", "dL_dopacities"), ("col", "dL_dcolors"), ("sca", "dL_dscales"), ("rot", "dL_drotations"),
                        ("cov", "dL_dcov3D"), ("sh", "dL_dshs")):
            if b[name] is not None:
                sums[k] = sums.get(k, 0.0) + b[name].astype(np.float64)
        m2.append(b["dL_dmeans2D"][:, :2].astype(np.float64))
        cam["view"].append(b["dL_dviewmatrix"])
        cam["proj"].append(b["dL_dprojmatrix"])
        cam["campos"].append(b["dL_dcampos"])
    if case.forward_only:
        return out
    out.update(sums, m2=np.stack(m2), **{k: np.stack(a) for k, a in cam.items()})
    if case.raw is not None:
        sc_r, ro_r, op_r, fd_r, ex_r = case.raw
        with np.errstate(invalid="ignore"):
            a = OA.backward(case.means3D, fd_r, np.zeros((P, 0, 3), F32), sc_r, ro_r, op_r, ex_r, np.zeros(3, F32), 0,
                            out.pop("sca"), out.pop("rot"), out.pop("op"), out.pop("col"))
        out.update(scaling=a["d_scaling"], rotation=a["d_rotation"], opacity=a["d_opacity"], f_dc=a["d_f_dc"], extra=a["d_extras"])
    for k in GRADS:
        out.setdefault(k, None)
    return out


# =================================================================================================================================
# deviations and bounds
# =================================================================================================================================
DECISIONS = ("ok", "radii", "tiles", "num_rendered")
RECORDS = ("pix", "tz", "conic")
CAMERA = ("view", "proj", "campos")


def outputs(case, ref):
    """the float outputs a case is compared on"""
    if case.forward_only:
        return list(RECORDS)
    return list(RECORDS) + [k for k in GRADS if ref.get(k) is not None] + ["m2"] + list(CAMERA)


def deviation(case, name, got, ref, per_row=False):
    """The deviation of output `name` in the unit its bound is stated in: the largest |got - ref| of a row over the row's largest
    reference element (pix: over the frame's larger side; a camera tensor: per view over its largest entry).  A row whose
    reference is exactly zero must be exactly zero: inf otherwise."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    # rows: every element of tz [V,P]; (view, Gaussian) of pix, conic, m2 [V,P,k]; the Gaussian of a parameter gradient [P,...]; the view
    # of a camera tensor [V,...]
    lead = ref.size if name == "tz" else (ref.shape[0] * ref.shape[1] if name in ("pix", "conic", "m2") else ref.shape[0])
    g2, r2 = got.reshape(lead, -1), ref.reshape(lead, -1)
    err = np.abs(g2 - r2).max(axis=1)
    err = np.where(np.isnan(err), np.inf, err)
    scale = np.abs(r2).max(axis=1)
    if name == "pix":
        scale = np.where(scale > 0, float(max(case.W, case.H)), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
    if per_row:
        return rel
    return float(rel.max()) if rel.size else 0.0


def floor(case, name):
    if name in N:
        return N[name] * U
    # (the camera tensors: the same n, per entry); kappa-fold for what passes through det, where the case says so
    return N_GRAD * U * (case_kappa(case) if case.kappa_scaled and name in THROUGH_DET else 1.0)


def bound(case, name, e_oracle):
    return max(MARGIN * e_oracle, floor(case, name))


_SENS = {}


def sensitivity(case):
    """{record: {output: per row (the rows of `deviation`)}}: how far the reference's gradients move when a forward record moves by
    its own floor — pix by N["pix"] 2^-24 of the frame (x and y summed), a conic entry by N["conic"] 2^-24 of its row (the three
    summed), tz by N["tz"] 2^-24.  First order: it scales with the size of the move."""
    if case.name not in _SENS:
        ref = reference(case)
        tot = {rec: {} for rec in RECORDS}
        for perturb in (("pix", 0), ("pix", 1), ("tz", 0), ("conic", 0), ("conic", 1), ("conic", 2)):
            r = reference(case, perturb=perturb)
            for k in outputs(case, ref):
                if k not in RECORDS:
                    d = deviation(case, k, r[k], ref[k], per_row=True)
                    tot[perturb[0]][k] = tot[perturb[0]].get(k, 0.0) + np.where(np.isfinite(d), d, 0.0)
        _SENS[case.name] = tot
    return _SENS[case.name]


def oracle_bound(case, name, e_oracle):
    """Per row: what the ORACLE may deviate by from the reference (the device's bound is `bound`).  A record: its floor.  A gradient: the
    floor plus the first-order effect of the oracle's own record errors e_oracle[record] — it differentiates in float64, but FROM its
    float32 records (a loss pixel one deviation from a centre known to 4e-6 px moves dL/dmeans2D by 8e-6 / sigma of itself)."""
    if name in RECORDS:
        return floor(case, name)
    s = sensitivity(case)
    return floor(case, name) + sum(s[rec][name] * (e_oracle[rec] / floor(case, rec)) for rec in RECORDS)


def oracle_errors(case):
    ref, orc = reference(case), oracle_run(case)
    return {k: deviation(case, k, orc[k], ref[k]) for k in outputs(case, ref)}


def decisions_differ(a, b):
    return [k for k in DECISIONS if not np.array_equal(np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64))]


def exceeds(dev, bnd):
    return not (dev <= bnd)


def structural_zeros(view, proj):
    """the entries no Gaussian writes: dV[4c + 3] and dPM[4c + 2]"""
    return np.asarray(view)[..., :, 3], np.asarray(proj)[..., :, 2]
