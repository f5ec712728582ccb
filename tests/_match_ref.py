"""Plain-torch reference of ufm_amd.matching.extract_matches (the contract of ufm_match_consistency in include/ufm_hip.h),
one image at a time, on the CPU in fp32, with the kernel's order of operations so that integer-exact cases agree bit for bit."""

import numpy as np
import torch


def consistency(F, Cs, G, Ct, tau_c=0.5, tau_e=1.0):
    """F (2, Hs, Ws), Cs (Hs, Ws), G (2, Ht, Wt), Ct (Ht, Wt) fp32 -> (s, e, valid, q): score (0 where not valid), cycle error
    (+inf where q leaves the box), validity, and q = p + F(p) as (2, Hs, Ws)."""
    F, Cs, G, Ct = (t.detach().float().cpu() for t in (F, Cs, G, Ct))
    Hs, Ws = Cs.shape
    Ht, Wt = Ct.shape
    ys, xs = torch.meshgrid(torch.arange(Hs, dtype=torch.float32), torch.arange(Ws, dtype=torch.float32), indexing="ij")
    qx, qy = xs + F[0], ys + F[1]
    inbox = (qx >= 0) & (qx <= Wt - 1) & (qy >= 0) & (qy <= Ht - 1)
    qxc, qyc = torch.where(inbox, qx, torch.zeros(())), torch.where(inbox, qy, torch.zeros(()))
    x0 = torch.floor(qxc).long().clamp(max=max(Wt - 2, 0))
    y0 = torch.floor(qyc).long().clamp(max=max(Ht - 2, 0))
    x1, y1 = (x0 + 1).clamp(max=Wt - 1), (y0 + 1).clamp(max=Ht - 1)
    wx, wy = qxc - x0.float(), qyc - y0.float()
    finite = torch.isfinite(F[0]) & torch.isfinite(F[1]) & torch.isfinite(Cs)

    def sample(v):
        nonlocal finite
        v00, v01, v10, v11 = v[y0, x0], v[y0, x1], v[y1, x0], v[y1, x1]
        finite = finite & torch.isfinite(v00) & torch.isfinite(v01) & torch.isfinite(v10) & torch.isfinite(v11)
        return (1 - wy) * ((1 - wx) * v00 + wx * v01) + wy * ((1 - wx) * v10 + wx * v11)

    gx, gy, ct = sample(G[0]), sample(G[1]), sample(Ct)
    dx, dy = (qxc + gx) - xs, (qyc + gy) - ys
    e = torch.where(inbox, torch.sqrt(dx * dx + dy * dy), torch.full((), float("inf")))
    valid = inbox & finite & (Cs >= tau_c) & (ct >= tau_c) & (e <= tau_e)
    s = torch.where(valid, Cs * ct / (1 + e), torch.zeros(()))
    s = torch.where(s == 0, torch.zeros(()), s)  # -0 -> +0, as the kernel's key does
    return s, e, valid, torch.stack([qx, qy])


def select(s, valid, q, cell, K):
    """Per-cell best valid pixel (largest s, then lowest index), then the K best of those -> (matches (K, 4), scores (K,), count)."""
    Hs, Ws = s.shape
    sv, vv = s.numpy().reshape(-1), valid.numpy().reshape(-1)
    idx = np.arange(Hs * Ws)
    ncx = (Ws + cell - 1) // cell
    cid = (idx // Ws // cell) * ncx + (idx % Ws) // cell
    keep = np.nonzero(vv)[0]
    order = keep[np.lexsort((keep, -sv[keep].astype(np.float64), cid[keep]))]  # by cell, then score down, then index up
    first = np.ones(len(order), bool)
    first[1:] = cid[order[1:]] != cid[order[:-1]]
    cand = order[first]
    cand = cand[np.lexsort((cand, -sv[cand].astype(np.float64)))][:K]
    n = len(cand)
    matches = np.full((K, 4), np.nan, np.float32)
    scores = np.zeros(K, np.float32)
    qv = q.numpy().reshape(2, -1)
    matches[:n, 0], matches[:n, 1] = cand % Ws, cand // Ws
    matches[:n, 2], matches[:n, 3] = qv[0, cand], qv[1, cand]
    scores[:n] = sv[cand]
    return matches, scores, n


def extract_matches(flow_st, covis_s, flow_ts, covis_t, num_matches=5000, cell=8, covisibility_threshold=0.5, cycle_threshold_px=1.0):
    """Batched reference: (matches (B, K, 4), scores (B, K), counts (B,)) as numpy arrays."""
    out = []
    for b in range(flow_st.shape[0]):
        s, e, valid, q = consistency(flow_st[b], covis_s[b], flow_ts[b], covis_t[b], covisibility_threshold, cycle_threshold_px)
        out.append(select(s, valid, q, cell, num_matches))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32)
