"""Sparse matches from dense flow: forward-backward consistency, one candidate per grid cell, top-K -- on the device.

``extract_matches`` takes the dense outputs of both directions (``predict_correspondences_batched(src, tgt)`` and
``(tgt, src)``) and returns a fixed-shape ``UFMMatchesOutput``; ``UniFlowMatchModelsBase.predict_matches`` runs the model in
both directions and calls it.  The contract (bilinear sampling on pixel indices, validity, score, cells, ties, padding) is the
comment of ``ufm_match_consistency`` in ``include/ufm_hip.h``; the kernels are ``ufm_amd/csrc/matches.hip``.
"""

from __future__ import annotations

from typing import Tuple

import torch

from . import hip
from .base import UFMMatchesOutput


def _check_inputs(flow_st, covis_s, flow_ts, covis_t) -> Tuple[torch.Tensor, ...]:
    ts = []
    for name, t in (("flow_st", flow_st), ("covis_s", covis_s), ("flow_ts", flow_ts), ("covis_t", covis_t)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 device tensor (ufm_amd has no CPU path)")
        ts.append(t.contiguous())
    flow_st, covis_s, flow_ts, covis_t = ts
    if covis_s.dim() == 4 and covis_s.shape[1] == 1:
        covis_s = covis_s.squeeze(1)
    if covis_t.dim() == 4 and covis_t.shape[1] == 1:
        covis_t = covis_t.squeeze(1)
    if flow_st.dim() != 4 or flow_st.shape[1] != 2 or flow_ts.dim() != 4 or flow_ts.shape[1] != 2:
        raise ValueError("flows must be (B, 2, H, W)")
    B, _, Hs, Ws = flow_st.shape
    Ht, Wt = flow_ts.shape[2:]
    if flow_ts.shape[0] != B or tuple(covis_s.shape) != (B, Hs, Ws) or tuple(covis_t.shape) != (B, Ht, Wt):
        raise ValueError(f"shapes disagree: flow_st {tuple(flow_st.shape)}, covis_s {tuple(covis_s.shape)}, "
                         f"flow_ts {tuple(flow_ts.shape)}, covis_t {tuple(covis_t.shape)}")
    if len({t.device for t in (flow_st, covis_s, flow_ts, covis_t)}) != 1:
        raise ValueError("all inputs must be on one device")
    return flow_st, covis_s, flow_ts, covis_t


def consistency_maps(flow_st, covis_s, flow_ts, covis_t, cell=8, covisibility_threshold=0.5, cycle_threshold_px=1.0):
    """The dense per-pixel maps of the consistency pass: score s (B, Hs, Ws), 0 where the pixel is not valid, and cycle
    error e (B, Hs, Ws), +inf where p + F(p) leaves the target image."""
    flow_st, covis_s, flow_ts, covis_t = _check_inputs(flow_st, covis_s, flow_ts, covis_t)
    B, _, Hs, Ws = flow_st.shape
    with torch.cuda.device(flow_st.device):
        ws = torch.empty(hip.match_ws_bytes(B, Hs, Ws, cell, 1), dtype=torch.uint8, device=flow_st.device)
        score = torch.empty((B, Hs, Ws), dtype=torch.float32, device=flow_st.device)
        err = torch.empty_like(score)
        hip.match_consistency(flow_st, covis_s, flow_ts, covis_t, cell, covisibility_threshold, cycle_threshold_px, ws, score, err)
    return score, err


def extract_matches(flow_st, covis_s, flow_ts, covis_t, num_matches=5000, cell=8, covisibility_threshold=0.5,
                    cycle_threshold_px=1.0) -> UFMMatchesOutput:
    """Top-``num_matches`` forward-backward consistent matches per image.

    flow_st (B, 2, Hs, Ws) / covis_s (B, Hs, Ws): source -> target flow and source covisibility; flow_ts (B, 2, Ht, Wt) /
    covis_t (B, Ht, Wt): target -> source.  fp32 device tensors in the original image frames (what
    ``predict_correspondences_batched`` returns).  A source pixel p is kept when q = p + F(p) lies in the target, both
    covisibilities reach ``covisibility_threshold`` and the cycle error |q + G(q) - p| is at most ``cycle_threshold_px``;
    its score is Cs(p) Ct(q) / (1 + e).  The best pixel of each ``cell`` x ``cell`` block is a candidate, and the
    ``num_matches`` best candidates come back sorted by score (ties: lower y * Ws + x first):
    matches (B, K, 4) = [xs, ys, xt, yt], scores (B, K), counts (B,) int32; rows past counts[b] are NaN / 0."""
    flow_st, covis_s, flow_ts, covis_t = _check_inputs(flow_st, covis_s, flow_ts, covis_t)
    B, _, Hs, Ws = flow_st.shape
    K = int(num_matches)
    dev = flow_st.device
    with torch.cuda.device(dev):
        ws = torch.empty(hip.match_ws_bytes(B, Hs, Ws, int(cell), K), dtype=torch.uint8, device=dev)
        matches = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
        scores = torch.empty((B, K), dtype=torch.float32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        hip.match_consistency(flow_st, covis_s, flow_ts, covis_t, int(cell), covisibility_threshold, cycle_threshold_px, ws)
        hip.match_topk(flow_st, int(cell), K, ws, matches, scores, counts)
    return UFMMatchesOutput(matches=matches, scores=scores, counts=counts)
