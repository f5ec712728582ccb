"""Sparse match extraction, CPU side: the plain-torch reference of the contract (tests/_match_ref.py) on hand-computed
cases, argument validation of the two C entry points (rejected on the host, nothing launched), and the CLI flag."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import _match_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def identity_pair(H, W, cov=1.0):
    z = torch.zeros(2, H, W)
    return z, torch.full((H, W), cov), z.clone(), torch.full((H, W), cov)


def test_reference_identity_flow_is_valid_everywhere_with_zero_error():
    F, Cs, G, Ct = identity_pair(5, 7, cov=0.75)
    s, e, valid, q = ref.consistency(F, Cs, G, Ct, 0.5, 1.0)
    assert valid.all() and (e == 0).all()
    assert (s == 0.75 * 0.75).all()
    m, sc, n = ref.select(s, valid, q, 1, 100)
    assert n == 35
    # equal scores everywhere: the lowest indices first, in order
    assert np.array_equal(m[:n, 0], np.arange(35) % 7) and np.array_equal(m[:n, 1], np.arange(35) // 7)
    assert np.array_equal(m[:n, 2:], m[:n, :2])


def test_reference_one_pixel_past_the_right_edge_is_invalid():
    F, Cs, G, Ct = identity_pair(4, 6)
    F[0] = 1.0  # q = (x + 1, y): the last column lands on x = Wt, outside [0, Wt - 1]
    G[0] = -1.0
    s, e, valid, q = ref.consistency(F, Cs, G, Ct, 0.5, 1.0)
    assert not valid[:, 5].any() and math.isinf(e[0, 5].item())
    assert valid[:, :5].all() and (e[:, :5] == 0).all()
    F[0, 0, 5] = 0.0  # exactly on the last column: valid (the box is closed)
    G[0, 0, 5] = 0.0
    s, e, valid, q = ref.consistency(F, Cs, G, Ct, 0.5, 1.0)
    assert valid[0, 5]


def test_reference_cycle_error_and_score_by_hand():
    F, Cs, G, Ct = identity_pair(3, 4, cov=1.0)
    F[0, 1, 1] = 0.5                     # q = (1.5, 1)
    G[0, 1, 1], G[0, 1, 2] = -0.1, -0.3  # G_x(q) = (-0.1 - 0.3) / 2 = -0.2 -> q + G - p = (0.3, 0)
    s, e, valid, q = ref.consistency(F, Cs, G, Ct, 0.5, 1.0)
    assert abs(e[1, 1].item() - 0.3) < 1e-6 and abs(s[1, 1].item() - 1 / 1.3) < 1e-6
    s, e, valid, q = ref.consistency(F, Cs, G, Ct, 0.5, 0.25)  # cycle threshold below the error
    assert not valid[1, 1]


def test_reference_non_finite_values_are_never_valid():
    F, Cs, G, Ct = identity_pair(4, 4)
    F[1, 0, 3] = float("nan")
    Cs[0, 1] = float("inf")
    G[0, 0, 0] = float("nan")  # a corner of pixel (0, 0) only
    Ct[3, 0] = float("nan")    # a corner of (2, 0) and (3, 0): read with zero weight by (2, 0), which still counts
    s, e, valid, q = ref.consistency(F, Cs, G, Ct, 0.0, float("inf"))
    bad = {(0, 3), (0, 1), (0, 0), (2, 0), (3, 0)}
    for y in range(4):
        for x in range(4):
            assert bool(valid[y, x]) == ((y, x) not in bad), (y, x)


def test_reference_tie_rule_within_and_across_cells():
    H, W = 6, 6
    F, Cs, G, Ct = identity_pair(H, W)
    s, e, valid, q = ref.consistency(F, Cs, G, Ct, 0.5, 1.0)
    m, sc, n = ref.select(s, valid, q, 3, 10)
    # four cells, constant score: each cell's top-left pixel, the cells in index order of those pixels
    assert n == 4
    assert m[:n, :2].tolist() == [[0, 0], [3, 0], [0, 3], [3, 3]]
    Cs[4, 5] = 0.9  # a lower score in cell (1, 1) does not change its pick
    s, e, valid, q = ref.consistency(F, Cs, G, Ct, 0.5, 1.0)
    m, sc, n = ref.select(s, valid, q, 3, 10)
    assert m[3, :2].tolist() == [3, 3]
    Cs[3:, 3:] = 0.6  # now (5, 4) is the best of that cell, and ranks last
    Cs[4, 5] = 0.9
    s, e, valid, q = ref.consistency(F, Cs, G, Ct, 0.5, 1.0)
    m, sc, n = ref.select(s, valid, q, 3, 10)
    assert m[3, :2].tolist() == [5, 4] and sc[3] == np.float32(0.9)


def test_reference_pads_when_there_are_fewer_candidates_than_k():
    F, Cs, G, Ct = identity_pair(4, 4)
    Cs[:2] = 0.1  # the top two rows fall under the covisibility threshold
    s, e, valid, q = ref.consistency(F, Cs, G, Ct, 0.5, 1.0)
    m, sc, n = ref.select(s, valid, q, 1, 12)
    assert n == 8
    assert np.isnan(m[8:]).all() and (sc[8:] == 0).all() and (sc[:8] == 1).all()
    assert m[0, :2].tolist() == [0, 2]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    if not os.path.exists(os.path.join(REPO, "ufm_amd", "libufm_hip.so")):
        g.build()
    from ufm_amd import hip

    return hip.lib()


def test_match_entry_points_reject_bad_arguments_without_a_launch(lib):
    P = ctypes.c_void_p(4096)  # fake device pointer: validation fails before anything could touch it
    ws = lib.ufm_match_ws_bytes(2, 32, 48, 4, 100)
    assert ws > 0
    assert lib.ufm_match_ws_bytes(1, 8, 8, 1, 0) == -1 and b"K=0" in lib.ufm_last_error()

    def topk(K=100, cell=4, flow=P, ws_bytes=ws, B=2):
        return lib.ufm_match_topk(flow, B, 32, 48, cell, K, P, ws_bytes, P, P, P, None)

    rc = topk(K=0)
    assert rc == -1 and b"K=0" in lib.ufm_last_error()
    rc = topk(K=8193)
    assert rc == -1 and b"K=8193" in lib.ufm_last_error()
    rc = topk(cell=0)
    assert rc == -1 and b"cell=0" in lib.ufm_last_error()
    rc = topk(flow=None)
    assert rc == -1 and b"null pointer" in lib.ufm_last_error()
    rc = topk(ws_bytes=ws - 8)
    assert rc == -1 and b"workspace" in lib.ufm_last_error()
    rc = topk(B=0)
    assert rc == -1 and b"B=0" in lib.ufm_last_error()

    def consistency(cell=4, covis=P, tau_c=0.5, tau_e=1.0, Ht=40, Wt=40):
        return lib.ufm_match_consistency(P, covis, P, P, 2, 32, 48, Ht, Wt, cell, tau_c, tau_e, P, ws, None, None, None)

    rc = consistency(cell=0)
    assert rc == -1 and b"cell=0" in lib.ufm_last_error()
    rc = consistency(covis=None)
    assert rc == -1 and b"null pointer" in lib.ufm_last_error()
    rc = consistency(Wt=0)
    assert rc == -1 and b"target shape" in lib.ufm_last_error()
    rc = consistency(tau_c=-0.5)
    assert rc == -1 and b"covisibility threshold" in lib.ufm_last_error()
    rc = consistency(tau_e=float("nan"))
    assert rc == -1 and b"cycle threshold" in lib.ufm_last_error()


def test_extract_matches_needs_device_tensors():
    from ufm_amd.matching import extract_matches

    F, Cs, G, Ct = identity_pair(4, 4)
    with pytest.raises(ValueError, match="device tensor"):
        extract_matches(F[None], Cs[None], G[None], Ct[None])


def test_cli_parser_accepts_matches():
    from ufm_amd import cli

    p = cli.build_parser()
    assert p.parse_args(["infer", "s.png", "t.png"]).matches is None
    a = p.parse_args(["infer", "s.png", "t.png", "--matches", "2000", "-o", "out"])
    assert (a.matches, a.output) == (2000, "out")
    with pytest.raises(SystemExit):
        p.parse_args(["infer", "s.png", "t.png", "--matches", "many"])


def test_predict_matches_needs_a_covisibility_output():
    from ufm_amd.base import UFMFlowFieldOutput, UFMOutputInterface, UniFlowMatchModelsBase

    class FlowOnly(UniFlowMatchModelsBase):
        def predict_correspondences_batched(self, source_image, target_image, data_norm_type=None):
            B, _, H, W = source_image.shape
            return UFMOutputInterface(flow=UFMFlowFieldOutput(flow_output=torch.zeros(B, 2, H, W)))

    img = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    for tgt in (img, torch.zeros(1, 3, 8, 6, dtype=torch.uint8)):  # the batched path and the two-call path
        with pytest.raises(ValueError, match="no covisibility"):
            FlowOnly().predict_matches(img, tgt)
