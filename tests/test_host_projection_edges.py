"""tests/projection_reference.py pinned on the host: every builder reaches the edge it is named for with unambiguous decisions, the
float64 statement of the projection is the one tests/torch_dense_ref.py composites with, the CPU oracle (oracle/splat_oracle.c: forward
AND hand-written backward, for the first time at the clamp and at the cull plane) takes the reference's decisions and lies within its
bound on every case, and every wrong model exceeds the device's bound on a case that names it, so that
tests/test_gpu_projection_edges.py cannot pass vacuously.  No test here touches a GPU."""
import numpy as np
import pytest
import torch

from tests import projection_reference as R
from tests.torch_dense_ref import render_dense

BACKWARD = R.case_names(backward=True)


@pytest.mark.parametrize("name", R.case_names())
def test_builder_reaches_its_edge(name):
    c = R.case(name)
    ref = R.reference(c)
    assert c.edge(ref) > 0, name
    assert R.ambiguous(c) == [], "a decision within 1e-4 of its threshold that is not exact in float32"
    assert R.ill_conditioned(c) == [], "a determinant that amplifies its inputs' roundings beyond the margin"
    assert c.W <= 48 and c.H <= 33 and (c.P <= 64 or name.startswith("block")) and 1 <= c.V <= 8
    if c.forward_only:
        return
    assert set(c.models) <= set(R.MODELS) and c.models
    for v in range(c.V):
        lit = {i for _, _, i in c.pixels[v]}
        assert lit == set(np.nonzero(ref["ok"][v])[0].tolist())               # every visible Gaussian, and no other, carries the loss
        assert all(1 <= sum(1 for p in c.pixels[v] if p[2] == i) <= 3 for i in lit)
        gc, gd, ga = c.grads[v]
        assert int((np.abs(gc).max(axis=0) > 0).sum()) == len(c.pixels[v]) == int((gd != 0).sum()) == int((ga != 0).sum())
    seen = ref["ok"].any(axis=0)
    assert (np.abs(ref["m3"]).max(axis=1) > 0)[seen].all()                  # a visible Gaussian carries a gradient
    assert not np.abs(ref["m3"])[~seen].any() and not np.abs(ref["m2"])[~ref["ok"]].any()


def test_clamp_and_cull_planes_are_reached():
    """the two counts that are zero over the rest of the suite"""
    clamped = {n: R._count_clamped(R.reference(R.case(n))) for n in BACKWARD}
    assert clamped["clamp x"] >= 6 and clamped["clamp y cov3D"] >= 6 and clamped["clamp xy modifier 1.6"] >= 3
    assert clamped["raw clamp x E 1"] >= 6 and clamped["window V 5"] >= 1 and clamped["window V 8"] >= 1
    for n in ("cull", "raw cull E 0"):
        below, above = R._count_near_plane(R.reference(R.case(n)))
        assert below >= 1 and above >= 1, n
    c = R.case("clamp x")
    ref = R.reference(c)
    lim = np.float32(1.3) * np.float32(c.tanfovx)
    txtz = (c.means3D[:, 0] / c.means3D[:, 2]).astype(np.float32)         # identity view, tz = 2: exact
    assert txtz[1] == lim and not ref["cx"][0, 1] and txtz[2] == np.nextafter(lim, np.float32(2)) and ref["cx"][0, 2]
    assert txtz[6] == -lim and not ref["cx"][0, 6] and ref["cx"][0, 7]
    tz = R.case("cull").means3D[:, 2]
    assert tz[0] == np.float32(0.2) and not ref_ok("cull")[0, 0] and tz[1] == np.nextafter(np.float32(0.2), np.float32(1)) and ref_ok("cull")[0, 1]


def ref_ok(name):
    return R.reference(R.case(name))["ok"]


@pytest.mark.parametrize("name", ["clamp xy modifier 1.6", "conic and radius", "channels 4", "sh degree 2"])
def test_reference_projection_is_the_dense_references(name):
    """project() (float32 thresholds and constants) against render_dense's own projection (double constants) where no Gaussian sits
    on a threshold: same radii, images to 1e-7"""
    c = R.case(name)
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    Vn, PMn, cpn = c.views[0]
    with torch.no_grad():
        color, depth, alpha, radii = render_dense(c.H, c.W, c.tanfovx, c.tanfovy, torch.tensor(c.bg), t(c.means3D), t(c.opacities), t(Vn),
                                                  t(PMn), t(cpn), colors_precomp=t(c.colors), shs=t(c.shs), sh_degree=c.sh_degree,
                                                  scales=t(c.scales), rotations=t(c.rotations), cov3D_precomp=t(c.cov), scale_modifier=c.mod)
        pr = R._projections(c)[0]
        color2, depth2, alpha2, _ = render_dense(c.H, c.W, c.tanfovx, c.tanfovy, torch.tensor(c.bg), t(c.means3D), t(c.opacities), t(Vn),
                                                 t(PMn), t(cpn), colors_precomp=t(c.colors), shs=t(c.shs), sh_degree=c.sh_degree, projection=pr)
    assert np.array_equal(radii.numpy(), R.reference(c)["radii"][0])
    for a, b in ((color, color2), (depth, depth2), (alpha, alpha2)):
        assert float((a - b).abs().max()) <= 1e-7 * max(1.0, float(a.abs().max()))


@pytest.mark.parametrize("name", R.case_names())
def test_oracle_takes_the_references_decisions_and_lies_within_its_bound(name):
    c = R.case(name)
    ref, orc = R.reference(c), R.oracle_run(c)
    assert R.decisions_differ(orc, ref) == []
    E = R.oracle_errors(c)
    for k in R.outputs(c, ref):
        dev = R.deviation(c, k, orc[k], ref[k], per_row=True)
        bnd = R.oracle_bound(c, k, E)
        assert (dev <= bnd).all(), (name, k, float((dev / bnd).max()))
    if c.forward_only:
        fin = np.isfinite(c.means3D).all(axis=1)
        assert not orc["ok"][0, ~fin].any() and orc["ok"][0, fin].all()
        return
    zv, zp = R.structural_zeros(orc["view"], orc["proj"])
    assert not zv.any() and not zp.any() and (c.shs is not None or not orc["campos"].any())


def _exposed(c, ref, E, wrong):
    """the outputs on which a wrong model leaves the device's bound (a decision: any difference)"""
    out = R.decisions_differ(wrong, ref)
    return out + [k for k in R.outputs(c, ref) if R.exceeds(R.deviation(c, k, wrong[k], ref[k]), R.bound(c, k, E[k]))]


@pytest.mark.parametrize("model", R.MODELS)
def test_every_wrong_model_exceeds_the_bound_of_a_case_that_names_it(model):
    named = [n for n in BACKWARD if model in R.case(n).models]
    assert named, model
    hits = {}
    for n in named:
        c = R.case(n)
        ref = R.reference(c)
        hits[n] = _exposed(c, ref, R.oracle_errors(c), R.reference(c, model=[model]))
    assert any(hits.values()), (model, hits)
    print(f"{R.MODEL_TEXT[model]}: " + "; ".join(f"{n}: {', '.join(h) or 'NOT exposed'}" for n, h in hits.items()))


@pytest.mark.parametrize("name", BACKWARD)
def test_no_case_is_so_loose_that_none_of_its_models_exceeds_it(name):
    c = R.case(name)
    ref, E = R.reference(c), R.oracle_errors(c)
    assert any(_exposed(c, ref, E, R.reference(c, model=[m])) for m in c.models), name


def test_the_reference_without_a_model_is_reproducible():
    c = R.case("clamp x")
    a, b = R.reference(c), R.reference(c, model=[])
    assert all(np.array_equal(a[k], b[k]) for k in ("m3", "m2", "sca", "rot", "view", "proj"))
