"""Sparse match extraction on the GPU (ufm_amd/csrc/matches.hip through ufm_amd.matching) against the plain-torch reference
of tests/_match_ref.py: dense score / cycle-error maps within 1e-5 relative, the selection exactly (order included) where the
inputs make the arithmetic exact, edges, non-finite inputs, the chunk-merge path, determinism, batch invariance, and the
model-level predict_matches / `ufm infer --matches` end to end on tiny random-init models."""
import numpy as np
import pytest
import torch

from tests import _match_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ufm_amd import hip

    hip.lib()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def affine_pair(B, Hs, Ws, Ht, Wt, seed, noise=0.05):
    """Smooth forward flows (a random affine map into the target frame) and their approximate inverses, plus noise."""
    g = gen(seed)
    F, G = torch.empty(B, 2, Hs, Ws), torch.empty(B, 2, Ht, Wt)
    for b in range(B):
        A = torch.eye(2) + 0.1 * torch.randn(2, 2, generator=g)
        A[0] *= max(Wt - 1, 1) / max(Ws - 1, 1)
        A[1] *= max(Ht - 1, 1) / max(Hs - 1, 1)
        t = torch.tensor([0.05 * Wt, 0.05 * Ht]) * torch.randn(2, generator=g)
        ys, xs = torch.meshgrid(torch.arange(Hs, dtype=torch.float32), torch.arange(Ws, dtype=torch.float32), indexing="ij")
        p = torch.stack([xs, ys]).reshape(2, -1)
        F[b] = (A @ p + t[:, None] - p).reshape(2, Hs, Ws)
        yt, xt = torch.meshgrid(torch.arange(Ht, dtype=torch.float32), torch.arange(Wt, dtype=torch.float32), indexing="ij")
        qt = torch.stack([xt, yt]).reshape(2, -1)
        G[b] = (torch.linalg.inv(A) @ (qt - t[:, None]) - qt).reshape(2, Ht, Wt)
    F += noise * torch.randn(F.shape, generator=g)
    G += noise * torch.randn(G.shape, generator=g)
    Cs = torch.rand(B, Hs, Ws, generator=g)
    Ct = torch.rand(B, Ht, Wt, generator=g)
    return F, Cs, G, Ct


def distinct_covis(B, H, W, seed):
    g = gen(seed)
    return torch.stack([(torch.randperm(H * W, generator=g).float() + 1) / (H * W) for _ in range(B)]).reshape(B, H, W)


def translation_pair(B, Hs, Ws, Ht, Wt, shifts, seed):
    """Integer translations (exact sampling, e = 0 where the pair overlaps) and all-distinct covisibilities."""
    F, G = torch.zeros(B, 2, Hs, Ws), torch.zeros(B, 2, Ht, Wt)
    for b, (tx, ty) in enumerate(shifts):
        F[b, 0], F[b, 1], G[b, 0], G[b, 1] = tx, ty, -tx, -ty
    return F, distinct_covis(B, Hs, Ws, seed), G, distinct_covis(B, Ht, Wt, seed + 1)


def run(F, Cs, G, Ct, **kw):
    from ufm_amd.matching import extract_matches

    out = extract_matches(F.to(DEV), Cs.to(DEV), G.to(DEV), Ct.to(DEV), **kw)
    torch.cuda.synchronize()
    return out.matches.cpu().numpy(), out.scores.cpu().numpy(), out.counts.cpu().numpy()


def assert_same_selection(F, Cs, G, Ct, **kw):
    m, s, c = run(F, Cs, G, Ct, **kw)
    rm, rs, rc = ref.extract_matches(F, Cs, G, Ct, **kw)
    np.testing.assert_array_equal(c, rc)
    np.testing.assert_array_equal(s, rs)
    np.testing.assert_array_equal(m, rm)  # NaN padding compares equal
    return m, s, c


@pytest.mark.parametrize("shape", [(37, 53, 37, 53), (40, 30, 55, 71), (9, 13, 1, 20), (9, 13, 17, 1), (6, 5, 1, 1)])
def test_dense_score_and_cycle_error_match_the_reference(shape):
    from ufm_amd.matching import consistency_maps

    Hs, Ws, Ht, Wt = shape
    F, Cs, G, Ct = affine_pair(2, Hs, Ws, Ht, Wt, seed=sum(shape))
    if Wt == 1:
        F[:, 0] = -torch.arange(Ws, dtype=torch.float32)  # land on the only column; the y flow stays random
    if Ht == 1:
        F[:, 1] = -torch.arange(Hs, dtype=torch.float32)[:, None]
    kw = dict(covisibility_threshold=0.2, cycle_threshold_px=2.0)
    s, e = consistency_maps(F.to(DEV), Cs.to(DEV), G.to(DEV), Ct.to(DEV), cell=4, **kw)
    s, e = s.cpu(), e.cpu()
    n_valid = 0
    for b in range(2):
        rs, re_, valid, _ = ref.consistency(F[b], Cs[b], G[b], Ct[b], kw["covisibility_threshold"], kw["cycle_threshold_px"])
        torch.testing.assert_close(e[b], re_, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(s[b], rs, rtol=1e-5, atol=1e-6)
        n_valid += int(valid.sum())
    assert n_valid > 0


@pytest.mark.parametrize("cell", [1, 3, 8])
def test_selection_is_exactly_the_reference(cell):
    shifts = [(3, -2), (-7, 5), (0, 0)]
    F, Cs, G, Ct = translation_pair(3, 45, 61, 50, 58, shifts, seed=cell)
    for K in (1, 50, 700):
        _, _, c = assert_same_selection(F, Cs, G, Ct, num_matches=K, cell=cell, covisibility_threshold=0.3)
        assert (c > 0).all()


def test_constant_score_selects_the_lowest_indices():
    H, W = 20, 30
    z = torch.zeros(1, 2, H, W)
    one = torch.ones(1, H, W)
    m, s, c = run(z, one, z, one, num_matches=100, cell=1)
    assert c[0] == 100 and (s[0] == 1).all()
    idx = np.arange(100)
    np.testing.assert_array_equal(m[0, :, 0], idx % W)
    np.testing.assert_array_equal(m[0, :, 1], idx // W)
    m, s, c = run(z, one, z, one, num_matches=100, cell=4)  # each cell's top-left pixel, cells in that pixel's index order
    want = sorted((y * W + x) for y in range(0, H, 4) for x in range(0, W, 4))
    assert c[0] == len(want)
    np.testing.assert_array_equal(m[0, : c[0], 1] * W + m[0, : c[0], 0], want)


def test_edges_of_the_target_box():
    Hs, Ws, Ht, Wt = 8, 10, 6, 7
    F, G = torch.zeros(1, 2, Hs, Ws), torch.zeros(1, 2, Ht, Wt)
    # every source pixel maps to one target point; G sends it back exactly where it is sampled
    ys, xs = torch.meshgrid(torch.arange(Hs, dtype=torch.float32), torch.arange(Ws, dtype=torch.float32), indexing="ij")
    tx = torch.full((Hs, Ws), 2.0)
    ty = torch.full((Hs, Ws), 3.0)
    tx[0, 0], ty[0, 0] = Wt - 1, 2.0                   # exactly on the last column: valid
    tx[0, 1], ty[0, 1] = 3.0, Ht - 1                   # exactly on the last row: valid
    tx[0, 2], ty[0, 2] = Wt - 1, Ht - 1                # the corner: valid
    tx[0, 3], ty[0, 3] = float(np.nextafter(np.float32(Wt - 1), np.float32(1e9))), 2.0   # just beyond the last column
    tx[0, 4], ty[0, 4] = 3.0, float(np.nextafter(np.float32(Ht - 1), np.float32(1e9)))   # just beyond the last row
    tx[0, 5], ty[0, 5] = -1e-6, 2.0                    # just before the first column
    tx[0, 6], ty[0, 6] = 1e30, 2.0                     # far outside
    tx[0, 7], ty[0, 7] = -3e38, -3e38
    tx[0, 8], ty[0, 8] = float("inf"), 1.0
    F[0, 0], F[0, 1] = tx - xs, ty - ys
    Cs = distinct_covis(1, Hs, Ws, 5) * 0.5 + 0.5
    Ct = torch.ones(1, Ht, Wt)
    m, s, c = run(F, Cs, G, Ct, num_matches=Hs * Ws, cell=1, cycle_threshold_px=float("inf"))
    rm, rs, rc = ref.extract_matches(F, Cs, G, Ct, num_matches=Hs * Ws, cell=1, cycle_threshold_px=float("inf"))
    # here e = |q - p| is not exact (sqrt, division): validity is compared exactly, scores to rounding
    np.testing.assert_array_equal(c, rc)
    order, rorder = np.argsort(m[0, : c[0], 1] * Ws + m[0, : c[0], 0]), np.argsort(rm[0, : rc[0], 1] * Ws + rm[0, : rc[0], 0])
    np.testing.assert_array_equal(m[0, : c[0]][order], rm[0, : rc[0]][rorder])
    np.testing.assert_allclose(s[0, : c[0]][order], rs[0, : rc[0]][rorder], rtol=1e-6)
    picked = set((m[0, : c[0], 1] * Ws + m[0, : c[0], 0]).astype(int).tolist())
    assert {0, 1, 2} <= picked and not picked & {3, 4, 5, 6, 7, 8}
    assert c[0] == Hs * Ws - 6


@pytest.mark.parametrize("where", ["F", "G", "Cs", "Ct"])
def test_nan_is_never_selected(where):
    F, Cs, G, Ct = translation_pair(1, 24, 24, 24, 24, [(1, 1)], seed=11)
    g = gen(12)
    t = {"F": F, "G": G, "Cs": Cs, "Ct": Ct}[where]
    flat = t.view(-1)
    hit = torch.randperm(flat.numel(), generator=g)[: flat.numel() // 5]
    flat[hit] = float("nan")
    m, s, c = assert_same_selection(F, Cs, G, Ct, num_matches=600, cell=1, covisibility_threshold=0.0)
    assert 0 < c[0] < 24 * 24
    assert np.isfinite(m[0, : c[0]]).all() and np.isfinite(s[0, : c[0]]).all()


def test_chunk_merge_path_against_the_reference():
    """1024 x 1024 with a cell per pixel: 64 chunks of 16 384 keys per image, six merge levels at K = 8192."""
    F, Cs, G, Ct = translation_pair(1, 1024, 1024, 1024, 1024, [(5, -3)], seed=21)
    _, _, c = assert_same_selection(F, Cs, G, Ct, num_matches=8192, cell=1, covisibility_threshold=0.1)
    assert c[0] == 8192
    F, Cs, G, Ct = translation_pair(2, 300, 200, 300, 200, [(1, 2), (-2, 0)], seed=22)  # 4 chunks, K not a power of two
    assert_same_selection(F, Cs, G, Ct, num_matches=5000, cell=1, covisibility_threshold=0.0)


def test_bitwise_repeatable_and_batch_invariant():
    F, Cs, G, Ct = affine_pair(3, 70, 90, 64, 80, seed=31)
    kw = dict(num_matches=300, cell=3, covisibility_threshold=0.1, cycle_threshold_px=1.5)
    a, b = run(F, Cs, G, Ct, **kw), run(F, Cs, G, Ct, **kw)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    one = run(F[1:2], Cs[1:2], G[1:2], Ct[1:2], **kw)
    for x, y in zip(a, one):
        assert x[1:2].tobytes() == y.tobytes()
    assert a[2][1] > 0


# --- model level: tiny random-init models (the build_pair pattern of the model tests, without the oracle) ------------------
def build_model(refine=False, res=(56, 56), seed=3):
    import ufm_amd
    from ufm_amd.modules import init_weights_

    cls = ufm_amd.UniFlowMatchClassificationRefinement if refine else ufm_amd.UniFlowMatchConfidence
    model = cls(**ufm_amd.ufm_tiny_config(resolution_wh=res, refine=refine)).eval()
    init_weights_(model, seed)
    return model.to(DEV)


def u8(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=gen(seed))


LOOSE = dict(num_matches=400, cell=2, covisibility_threshold=0.0, cycle_threshold_px=float("inf"))


def same(a, b):
    return all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in ((a.matches, b.matches), (a.scores, b.scores), (a.counts, b.counts)))


@pytest.mark.parametrize("refine", [False, True])
def test_predict_matches_equals_extract_matches_on_two_calls(refine):
    from ufm_amd.matching import extract_matches

    model = build_model(refine=refine)
    for src, tgt in (((2, 56, 56, 3), (2, 56, 56, 3)), ((2, 50, 60, 3), (2, 56, 44, 3))):  # one 2B batch; two calls
        s, t = u8(src, 1).to(DEV), u8(tgt, 2).to(DEV)
        got = model.predict_matches(s, t, **LOOSE)
        fwd = model.predict_correspondences_batched(s, t)
        bwd = model.predict_correspondences_batched(t, s)
        want = extract_matches(fwd.flow.flow_output, fwd.covisibility.mask, bwd.flow.flow_output, bwd.covisibility.mask, **LOOSE)
        assert same(got, want), (refine, src, tgt)
        assert got.matches.shape == (2, 400, 4) and (got.counts.cpu() > 0).all()
    # unbatched CHW inputs come back with a batch dim of 1
    one = model.predict_matches(u8((3, 56, 56), 4).to(DEV), u8((3, 56, 56), 5).to(DEV), **LOOSE)
    assert one.matches.shape == (1, 400, 4)


def test_ufm_infer_cli_writes_matches(tmp_path, monkeypatch, capsys):
    from PIL import Image

    from ufm_amd import cli

    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, (90, 120, 3), dtype=np.uint8)
    tgt = rng.integers(0, 256, (80, 110, 3), dtype=np.uint8)
    Image.fromarray(src).save(tmp_path / "s.png")
    Image.fromarray(tgt).save(tmp_path / "t.png")
    model = build_model()
    monkeypatch.setattr(cli, "load_model", lambda args: model.set_numerics(args.numerics))
    out = tmp_path / "out"
    cli.main(["infer", str(tmp_path / "s.png"), str(tmp_path / "t.png"), "-o", str(out), "--random-init", "--matches", "100"])
    printed = capsys.readouterr().out
    z = np.load(out / "matches.npz")
    n = z["matches"].shape[0]
    assert z["matches"].shape == (n, 4) and z["scores"].shape == (n,) and n <= 100
    assert f"matches.npz ({n} matches)" in printed
    want = model.predict_matches(torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV), num_matches=100)
    assert int(want.counts[0]) == n
    np.testing.assert_array_equal(z["matches"], want.matches[0, :n].cpu().numpy())
    np.testing.assert_array_equal(z["scores"], want.scores[0, :n].cpu().numpy())
    assert np.isfinite(z["matches"]).all() and (np.diff(z["scores"]) <= 0).all()
    for name in cli.ARTEFACTS:
        assert (out / name).exists()
