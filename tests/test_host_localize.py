"""Host-side checks of the localisation stage (splatloc_amd/localize.py, csrc/retrieval.hip): the numpy restatement
(tests/localize_reference.py) reproduces the reference fixture (tests/golden/localize.npz), the seeded cases hash to what the
fixture was made from, the retrieval file is the reference's byte for byte, and every argument error is raised before any
device work."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from splatloc_amd import _native
from splatloc_amd import localize as L
from tests import localize_reference as LR

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "localize.npz")
CASES = sorted(LR.RETRIEVAL_CASES)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("case", CASES)
def test_seeded_cases_hash_to_the_fixture(golden, case):
    q, db, k, draws = LR.retrieval_case(case)
    seed, Q, N, D, kk = (int(x) for x in golden[f"r{case}_shape"])
    assert (seed, Q, N, D, kk) == LR.RETRIEVAL_CASES[case] and q.shape == (Q, D) and db.shape == (N, D) and k == kk
    assert q.dtype == db.dtype == np.float32 and draws <= LR.MAX_REDRAWS
    assert LR.case_hash(q, db) == str(golden[f"r{case}_sha256"])


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_retrieval(golden, case):
    q, db, k, _ = LR.retrieval_case(case)
    idx, sims = LR.retrieval_topk(q, db, k)
    assert np.array_equal(idx, golden[f"r{case}_ind"])
    qn = np.sqrt((q.astype(np.float64) ** 2).sum(axis=1))
    dn = np.sqrt((db.astype(np.float64) ** 2).sum(axis=1))
    bound = LR.gamma(q.shape[1]) * qn[:, None] * dn[idx]
    err = np.abs(golden[f"r{case}_sims"].astype(np.float64) - sims)
    print(f"case {case}: max |sims - f64| / bound = {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)


def test_exact_cases_have_ties_and_a_stable_order():
    for which in (0, 1):
        q, db, k, idx, sims = LR.exact_case(which)
        assert k == L.MAX_K and idx.shape == (q.shape[0], k)
        assert np.all(sims[:, :-1] >= sims[:, 1:])
        tied = sims[:, :-1] == sims[:, 1:]
        assert tied.any(axis=1).all()                      # every row has ties: the rule decides
        assert np.all(idx[:, :-1][tied] < idx[:, 1:][tied])
        i2, s2 = LR.retrieval_topk(q, db, k)                # the f64 restatement is exact on integers too
        assert np.array_equal(i2, idx) and np.array_equal(s2.astype(np.float32), sims)


def test_restatement_reproduces_the_reference_pose_errors(golden):
    theta, dist = LR.pose_errors(golden["p_R_est"], golden["p_t_est"], golden["p_R_gt"], golden["p_t_gt"])
    ref_t, ref_d = golden["p_thetas"].reshape(-1).astype(np.float64), golden["p_dists"]
    assert golden["p_thetas"].shape == (400, 1, 1) and golden["p_thetas"].dtype == np.float32
    err = np.abs(theta.astype(np.float64) - ref_t)
    print("max |theta - ref| / bound =", float((err / LR.theta_bound(ref_t)).max()))
    assert np.all(err <= LR.theta_bound(ref_t))
    assert np.all(np.abs(dist - ref_d) <= 4 * np.spacing(ref_d))
    small = golden["p_angles"] <= 0.05
    assert small.sum() == 24 and np.all(np.abs(theta[small] - 0.05595291) < 1e-6)    # the reference's floor (acos' last bit is free)
    assert abs(float(theta[-1]) - 180.0) < 1e-3                                   # the half turn about z
    for R in (golden["p_R_est"], golden["p_R_gt"]):
        assert {LR.quat_branch(r) for r in R} == {1, 2, 3, 4}
    v = np.ones(400, bool)
    v[[0, 17, 399]] = False
    t2, d2 = LR.pose_errors(golden["p_R_est"], golden["p_t_est"], golden["p_R_gt"], golden["p_t_gt"], valid=v)
    assert np.isnan(t2[~v]).all() and np.isnan(d2[~v]).all() and np.array_equal(t2[v], theta[v])


def test_retrieval_file_is_the_references_and_round_trips(golden, tmp_path):
    _, Q, N, _, k = (int(x) for x in golden["r1_shape"])
    qn = [f"query_{i:04d}.jpg" for i in range(Q)]
    dn = [f"frame_{i:05d}.jpg" for i in range(N)]
    path = tmp_path / "netvlad_retrieval.txt"
    L.write_retrieval_file(path, qn, dn, golden["r1_ind"])
    assert open(path, "rb").read() == str(golden["r1_text"]).encode()
    L.write_retrieval_file(path, qn, dn, torch.from_numpy(golden["r1_ind"]))
    assert open(path, "rb").read() == str(golden["r1_text"]).encode()
    res = L.load_retrieval_results(path)
    assert list(res) == qn
    assert all(res[qn[i]] == [dn[j] for j in golden["r1_ind"][i]] for i in range(Q))
    with pytest.raises(ValueError, match="idx must be"):
        L.write_retrieval_file(path, qn[:-1], dn, golden["r1_ind"])
    with pytest.raises(ValueError, match="outside"):
        L.write_retrieval_file(path, qn, dn[:5], golden["r1_ind"])


def test_argument_errors_come_before_any_device_work(tmp_path):
    q, d = np.zeros((3, 8), np.float32), np.zeros((20, 8), np.float32)
    with pytest.raises(ValueError, match="must be \\[rows, D\\]"):
        L.retrieve(q[0], d)
    with pytest.raises(ValueError, match="must be \\[rows, D\\]"):
        L.retrieve(q, d[None])
    with pytest.raises(ValueError, match="dimensions differ"):
        L.retrieve(q, np.zeros((20, 9), np.float32))
    for k in (0, -1, 21, 129):
        with pytest.raises(ValueError, match="must lie in"):
            L.retrieve(q, np.zeros((200, 8), np.float32) if k == 129 else d, k=k)
    with pytest.raises(ValueError, match="float16, float32 or float64"):
        L.retrieve(q.astype(np.int32), d)
    with pytest.raises(ValueError, match="at least one"):
        L.retrieve(np.zeros((3, 0), np.float32), np.zeros((20, 0), np.float32))
    with pytest.raises(ValueError, match="at least one"):
        L.retrieve(q, np.zeros((0, 8), np.float32))
    with pytest.raises(ValueError, match="descriptors for"):
        L.generate_retrieval_file(q, d, ["a", "b"], [str(i) for i in range(20)], tmp_path / "x.txt")
    R, t = np.tile(np.eye(3), (4, 1, 1)), np.zeros((4, 3))
    with pytest.raises(ValueError, match="R \\[B, 3, 3\\]"):
        L.pose_errors(R[0], t, R, t)
    with pytest.raises(ValueError, match="R \\[B, 3, 3\\]"):
        L.pose_errors(R, t[:3], R, t)
    with pytest.raises(ValueError, match="4 estimated and 3"):
        L.pose_errors(R, t, R[:3], t[:3])
    with pytest.raises(ValueError, match="valid must hold"):
        L.pose_errors(R, t, R, t, valid=np.ones(3, bool))
    with pytest.raises(ValueError, match="floating point"):
        L.pose_errors(R.astype(np.int64), t, R, t)
    cam = {"model": "OPENCV", "width": 64, "height": 48, "params": [40.0, 40.0, 31.5, 23.5, 0, 0, 0, 0]}
    with pytest.raises(ValueError, match="distortion"):
        L.Localizer(None, None, None, np.eye(3), 64, 48, dict(cam, params=[40.0, 40.0, 31.5, 23.5, 0.1, 0, 0, 0]))
    with pytest.raises(ValueError, match="subset must be"):
        L.Localizer(None, None, None, np.eye(3), 64, 48, cam, subset=np.zeros((5, 2)))
    loc = L.Localizer(None, None, None, np.eye(3), 64, 48, cam)
    one = {"keypoints": np.zeros((6, 2), np.float32), "descriptors": np.zeros((16, 6), np.float32)}
    with pytest.raises(ValueError, match="1 queries and 2"):
        loc.localize([one], [{}], [0, 0])
    with pytest.raises(ValueError, match="outside"):
        loc.localize([one], [{}], [1])
    with pytest.raises(ValueError, match="keypoints must be \\[n, 2\\]"):
        loc.localize([dict(one, descriptors=np.zeros((16, 5), np.float32))], [{}], [0])
    with pytest.raises(ValueError, match="must be finite"):
        loc.localize([dict(one, keypoints=np.full((6, 2), np.nan, np.float32))], [{}], [0])


@pytest.mark.skipif(torch.cuda.is_available(), reason="the message of a machine without a device")
def test_without_a_device_the_calls_raise():
    q, d = np.zeros((3, 8), np.float32), np.zeros((20, 8), np.float32)
    with pytest.raises(RuntimeError, match="no HIP device"):
        L.retrieve(q, d, k=5)
    R, t = np.tile(np.eye(3), (4, 1, 1)), np.zeros((4, 3))
    with pytest.raises(RuntimeError, match="no HIP device"):
        L.pose_errors(R, t, R, t)
    with pytest.raises(RuntimeError, match="no HIP device"):
        L.eval_pose(torch.from_numpy(R), torch.from_numpy(t), torch.from_numpy(R), torch.from_numpy(t))


def test_workspace_never_grows_with_the_similarity_matrix():
    lib = _native.load()
    assert _native.ABI_VERSION == 20 and lib.splatraster_abi_version() == 20
    ws = lib.splatraster_retrieval_workspace_bytes
    assert ws(1000, 100000, 4096, 10) < 1000 * 100000 * 4 // 8
    # per-slice lists only: at most 64 slices of k eight-byte keys per query, whatever N and D are
    for Q, N, D, k in ((1000, 100000, 4096, 10), (1, 1 << 30, 128, 128), (900, 180, 4096, 10), (37, 20000, 4096, 10)):
        assert ws(Q, N, D, k) <= Q * 64 * k * 8 + 256
        assert ws(Q, 10 * N if N < 1 << 27 else N, D, k) <= Q * 64 * k * 8 + 256
    assert ws(0, 100, 16, 5) == 0 and ws(5, 100, 16, 200) == 0


def test_bad_retrieval_arguments_return_the_status_without_a_launch():
    lib = _native.load()
    st = C.c_int32(7)   # host memory: a launch or a memset would fault on it, the argument check returns first
    p = C.cast(C.pointer(st), C.c_void_p)
    for Q, N, D, k in ((1, 10, 8, 0), (1, 10, 8, 11), (1, 200, 8, 129), (1, 10, 0, 1), (-1, 10, 8, 1), (1, 0, 8, 1),
                       (1, 1 << 31, 8, 1)):
        assert lib.splatraster_retrieval_topk(Q, N, D, k, p, p, p, p, p, p, None) == 1
    assert lib.splatraster_retrieval_topk(1, 10, 8, 1, None, None, None, None, None, None, None) == 1
    assert lib.splatraster_pose_errors(-1, *([None] * 8)) == 1 and lib.splatraster_pose_errors(0, *([None] * 8)) == 0
    assert lib.splatraster_pose_errors(3, *([None] * 8)) == 1
    assert lib.splatraster_pose_invert(-1, *([None] * 5)) == 1 and lib.splatraster_pose_invert(0, *([None] * 5)) == 0
    assert st.value == 7
