// Sparse match extraction with forward-backward consistency (ufm_amd/matching.py::extract_matches): the "match + sample"
// step of a dense matcher, kept on the device.  Two stages:
//   1. match_consistency_kernel -- one pass over the source pixels: sample the target->source flow G and the target
//      covisibility Ct bilinearly at q = p + F(p), cycle error e = |q + G(q) - p|, validity, score
//      s = Cs(p) * Ct(q) / (1 + e), and the per-cell maximum of the packed key
//          key = float_bits(s) << 32 | (0xFFFFFFFF - idx),   idx = y * Ws + x
//      (s >= 0, so the unsigned maximum is "largest score, then lowest index"; 0 = no candidate).  The wave reduces its
//      lanes' keys per cell with cross-lane shuffles, then one integer atomicMax per cell segment: deterministic.
//   2. top-K of each image's cell keys: chunks of up to 16 384 keys sorted descending in LDS by a bitonic sort
//      (16 384 x 8 B = 128 KiB of the 160 KiB LDS), each reduced to its top L = pow2ceil(K) keys; pairs of lists merged
//      (half-cleaner + bitonic merge of the top half, 2L <= 16 384) until one list per image remains; then the rows of
//      matches / scores / counts are written from it (padding: NaN rows, score 0).
// The contract (sampling, validity, ties) is stated in include/ufm_hip.h and pinned by tests/test_matches_*.py.
#include "common.h"

namespace {

constexpr int CHUNK = 16384;    // keys sorted by one workgroup (128 KiB of LDS)
constexpr int MAXK = 8192;      // 2 * pow2ceil(K) <= CHUNK: a pair of lists fits one workgroup's LDS
constexpr int SORT_THREADS = 1024;

__host__ __device__ inline int pow2ceil(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

__device__ __forceinline__ bool finite(float v) { return __builtin_isfinite(v); }

// v = (1-wy)((1-wx) v00 + wx v01) + wy((1-wx) v10 + wx v11), in this order (the reference of the tests evaluates it the same way)
__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, float wx, float wy) {
    return (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
}

__global__ __launch_bounds__(256) void match_consistency_kernel(const float* __restrict__ F, const float* __restrict__ Cs,
                                                                const float* __restrict__ G, const float* __restrict__ Ct,
                                                                int Hs, int Ws, int Ht, int Wt, int cell, int ncx, int ncells,
                                                                float tau_c, float tau_e, unsigned long long* __restrict__ keys,
                                                                float* __restrict__ score, float* __restrict__ err) {
    const int b = blockIdx.y;
    const long long HWs = (long long)Hs * Ws, HWt = (long long)Ht * Wt;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    F += (size_t)b * 2 * HWs, Cs += (size_t)b * HWs, G += (size_t)b * 2 * HWt, Ct += (size_t)b * HWt;
    unsigned long long key = 0;
    int cid = -1 - (int)(threadIdx.x & 63);  // lanes past the image: a segment of their own each, no key
    if (t < HWs) {
        const int y = (int)(t / Ws), x = (int)(t - (long long)y * Ws);
        cid = (y / cell) * ncx + x / cell;
        const float fx = F[t], fy = F[HWs + t], cs = Cs[t];
        const float qx = (float)x + fx, qy = (float)y + fy;
        float s = 0.f, e = __builtin_inff();
        // the box test comes before any read of G / Ct (NaN fails it)
        if (qx >= 0.f && qx <= (float)(Wt - 1) && qy >= 0.f && qy <= (float)(Ht - 1)) {
            const int x0 = Wt == 1 ? 0 : min((int)floorf(qx), Wt - 2), y0 = Ht == 1 ? 0 : min((int)floorf(qy), Ht - 2);
            const int x1 = min(x0 + 1, Wt - 1), y1 = min(y0 + 1, Ht - 1);
            const float wx = qx - (float)x0, wy = qy - (float)y0;
            const size_t o00 = (size_t)y0 * Wt + x0, o01 = (size_t)y0 * Wt + x1, o10 = (size_t)y1 * Wt + x0, o11 = (size_t)y1 * Wt + x1;
            const float gx00 = G[o00], gx01 = G[o01], gx10 = G[o10], gx11 = G[o11];
            const float gy00 = G[HWt + o00], gy01 = G[HWt + o01], gy10 = G[HWt + o10], gy11 = G[HWt + o11];
            const float c00 = Ct[o00], c01 = Ct[o01], c10 = Ct[o10], c11 = Ct[o11];
            const float gx = bilerp(gx00, gx01, gx10, gx11, wx, wy), gy = bilerp(gy00, gy01, gy10, gy11, wx, wy);
            const float ct = bilerp(c00, c01, c10, c11, wx, wy);
            const float dx = (qx + gx) - (float)x, dy = (qy + gy) - (float)y;
            e = sqrtf(dx * dx + dy * dy);
            const bool all_finite = finite(fx) && finite(fy) && finite(cs) && finite(gx00) && finite(gx01) && finite(gx10) &&
                                    finite(gx11) && finite(gy00) && finite(gy01) && finite(gy10) && finite(gy11) && finite(c00) &&
                                    finite(c01) && finite(c10) && finite(c11);
            if (all_finite && cs >= tau_c && ct >= tau_c && e <= tau_e) {
                s = cs * ct / (1.f + e);
                unsigned bits = __float_as_uint(s);
                if (bits == 0x80000000u) bits = 0;  // -0 (a covisibility of -0 at tau_c = 0) orders as +0
                key = ((unsigned long long)bits << 32) | (0xFFFFFFFFu - (unsigned)t);
            }
        }
        if (score) score[(size_t)b * HWs + t] = s;
        if (err) err[(size_t)b * HWs + t] = e;
    }
    keys += (size_t)b * ncells;
    if (cell == 1) {  // a cell per pixel: every key is its cell's (zeros included, no memset, no atomics)
        if (t < HWs) keys[t] = key;
        return;
    }
    // segmented max over the wave's runs of equal cell id (consecutive pixels of a row share a cell): after the loop the
    // first lane of each run holds the run's maximum
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int ocid = __shfl_down(cid, off);
        const unsigned long long okey = __shfl_down(key, off);
        if (lane + off < 64 && ocid == cid && okey > key) key = okey;
    }
    const int prev = __shfl_up(cid, 1);
    if ((lane == 0 || prev != cid) && key != 0) atomicMax(keys + cid, key);
}

// descending bitonic sort of s[0, n), n a power of two, by all threads of the block
__device__ __forceinline__ void bitonic_sort_desc(unsigned long long* s, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < (n >> 1); p += blockDim.x) {
                const int i = 2 * p - (p & (j - 1)), l = i + j;  // i has bit j clear
                const unsigned long long a = s[i], c = s[l];
                const bool desc = (i & k) == 0;
                if (desc ? a < c : a > c) s[i] = c, s[l] = a;
            }
            __syncthreads();
        }
    }
}

// s[0, n) is bitonic -> descending, n a power of two
__device__ __forceinline__ void bitonic_merge_desc(unsigned long long* s, int n) {
    for (int j = n >> 1; j > 0; j >>= 1) {
        for (int p = threadIdx.x; p < (n >> 1); p += blockDim.x) {
            const int i = 2 * p - (p & (j - 1)), l = i + j;
            const unsigned long long a = s[i], c = s[l];
            if (a < c) s[i] = c, s[l] = a;
        }
        __syncthreads();
    }
}

// one chunk of image b's keys -> its top L keys, descending (zero padded)
__global__ __launch_bounds__(SORT_THREADS) void match_chunk_sort_kernel(const unsigned long long* __restrict__ keys, int ncells,
                                                                        int nchunks, int L, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s[CHUNK];
    const int c = blockIdx.x, b = blockIdx.y;
    const int base = c * CHUNK, n = min(CHUNK, ncells - base);
    const int N = max(pow2ceil(n), L);
    keys += (size_t)b * ncells + base;
    for (int i = threadIdx.x; i < N; i += blockDim.x) s[i] = i < n ? keys[i] : 0ull;
    __syncthreads();
    bitonic_sort_desc(s, N);
    out += ((size_t)b * nchunks + c) * L;
    for (int i = threadIdx.x; i < L; i += blockDim.x) out[i] = s[i];
}

// lists 2p and 2p+1 of image b (nin lists of L keys, descending) -> the top L of both, descending
__global__ __launch_bounds__(SORT_THREADS) void match_merge_kernel(const unsigned long long* __restrict__ in, int nin, int L,
                                                                   unsigned long long* __restrict__ out, int nout) {
    __shared__ unsigned long long s[MAXK];
    const int p = blockIdx.x, b = blockIdx.y;
    const unsigned long long* A = in + ((size_t)b * nin + 2 * p) * L;
    const unsigned long long* Bl = 2 * p + 1 < nin ? A + L : nullptr;
    // half-cleaner of the bitonic sequence A ++ reverse(B): the larger L keys, themselves a bitonic sequence
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        const unsigned long long a = A[i], c = Bl ? Bl[L - 1 - i] : 0ull;
        s[i] = a > c ? a : c;
    }
    __syncthreads();
    bitonic_merge_desc(s, L);
    out += ((size_t)b * nout + p) * L;
    for (int i = threadIdx.x; i < L; i += blockDim.x) out[i] = s[i];
}

__global__ __launch_bounds__(256) void match_write_kernel(const unsigned long long* __restrict__ top, int L, int K,
                                                          const float* __restrict__ F, int Hs, int Ws, float* __restrict__ matches,
                                                          float* __restrict__ scores, int* __restrict__ counts) {
    const int b = blockIdx.x;
    const long long HWs = (long long)Hs * Ws;
    top += (size_t)b * L, F += (size_t)b * 2 * HWs, matches += (size_t)b * K * 4, scores += (size_t)b * K;
    if (threadIdx.x == 0 && top[0] == 0) counts[b] = 0;
    for (int r = threadIdx.x; r < K; r += blockDim.x) {
        const unsigned long long key = top[r];
        float4 m = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        float sc = 0.f;
        if (key != 0) {
            const unsigned idx = 0xFFFFFFFFu - (unsigned)key;
            const int y = (int)(idx / (unsigned)Ws), x = (int)(idx - (unsigned)y * (unsigned)Ws);
            m = make_float4((float)x, (float)y, (float)x + F[idx], (float)y + F[HWs + idx]);
            sc = __uint_as_float((unsigned)(key >> 32));
            if (r == K - 1 || top[r + 1] == 0) counts[b] = r + 1;  // the last candidate row
        }
        reinterpret_cast<float4*>(matches)[r] = m;
        scores[r] = sc;
    }
}

struct MatchLayout {
    int ncx, ncells, L, nchunks;
    long long keys_bytes, list_bytes, total;
};

// UFM_ERR_ARG (message set) when the sizes break the contract
int match_layout(const char* who, int B, int Hs, int Ws, int cell, int K, MatchLayout* m) {
    UFM_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d must be in [1, 65535]", who, B);
    UFM_REQUIRE(Hs >= 1 && Ws >= 1 && (long long)Hs * Ws < (1ll << 31), "%s: bad source shape %dx%d", who, Hs, Ws);
    UFM_REQUIRE(cell >= 1, "%s: cell=%d must be >= 1", who, cell);
    UFM_REQUIRE(K >= 1 && K <= MAXK, "%s: K=%d must be in [1, %d]", who, K, MAXK);
    m->ncx = (Ws + cell - 1) / cell;
    m->ncells = (int)((long long)((Hs + cell - 1) / cell) * m->ncx);
    m->L = pow2ceil(K);
    m->nchunks = (m->ncells + CHUNK - 1) / CHUNK;
    m->keys_bytes = (long long)B * m->ncells * 8;
    m->list_bytes = (long long)B * m->nchunks * m->L * 8;
    // [keys][list ping][list pong]; the pong buffer holds at most ceil(nchunks / 2) lists
    m->total = m->keys_bytes + m->list_bytes + (long long)B * ((m->nchunks + 1) / 2) * m->L * 8;
    return UFM_OK;
}

}  // namespace

extern "C" int64_t ufm_match_ws_bytes(int B, int Hs, int Ws, int cell, int K) {
    MatchLayout m;
    if (match_layout("ufm_match_ws_bytes", B, Hs, Ws, cell, K, &m) != UFM_OK) return UFM_ERR_ARG;
    return m.total;
}

extern "C" int ufm_match_consistency(const float* flow_st, const float* covis_s, const float* flow_ts, const float* covis_t, int B, int Hs,
                                     int Ws, int Ht, int Wt, int cell, float covis_threshold, float cycle_threshold, void* ws,
                                     int64_t ws_bytes, float* score, float* err, void* stream) {
    UFM_REQUIRE(flow_st && covis_s && flow_ts && covis_t && ws, "ufm_match_consistency: null pointer");
    MatchLayout m;
    if (match_layout("ufm_match_consistency", B, Hs, Ws, cell, 1, &m) != UFM_OK) return UFM_ERR_ARG;
    UFM_REQUIRE(Ht >= 1 && Wt >= 1 && (long long)Ht * Wt < (1ll << 31), "ufm_match_consistency: bad target shape %dx%d", Ht, Wt);
    UFM_REQUIRE(covis_threshold >= 0.f, "ufm_match_consistency: covisibility threshold %g must be >= 0", covis_threshold);
    UFM_REQUIRE(cycle_threshold >= 0.f, "ufm_match_consistency: cycle threshold %g must be >= 0", cycle_threshold);
    UFM_REQUIRE(ws_bytes >= m.keys_bytes, "ufm_match_consistency: workspace of %lld bytes, %lld needed", (long long)ws_bytes, m.keys_bytes);
    unsigned long long* keys = (unsigned long long*)ws;
    if (cell > 1 && hipMemsetAsync(keys, 0, (size_t)m.keys_bytes, (hipStream_t)stream) != hipSuccess) {
        ufm_set_error("ufm_match_consistency: hipMemsetAsync failed");
        return UFM_ERR_LAUNCH;
    }
    const long long HWs = (long long)Hs * Ws;
    const dim3 grid((unsigned)((HWs + 255) / 256), B);
    hipLaunchKernelGGL(match_consistency_kernel, grid, dim3(256), 0, (hipStream_t)stream, flow_st, covis_s, flow_ts, covis_t, Hs, Ws, Ht, Wt,
                       cell, m.ncx, m.ncells, covis_threshold, cycle_threshold, keys, score, err);
    UFM_CHECK_LAUNCH("ufm_match_consistency");
    return UFM_OK;
}

extern "C" int ufm_match_topk(const float* flow_st, int B, int Hs, int Ws, int cell, int K, void* ws, int64_t ws_bytes, float* matches,
                              float* scores, int* counts, void* stream) {
    UFM_REQUIRE(flow_st && ws && matches && scores && counts, "ufm_match_topk: null pointer");
    MatchLayout m;
    if (match_layout("ufm_match_topk", B, Hs, Ws, cell, K, &m) != UFM_OK) return UFM_ERR_ARG;
    UFM_REQUIRE(((uintptr_t)matches & 15) == 0, "ufm_match_topk: matches must be 16-byte aligned");
    UFM_REQUIRE(ws_bytes >= m.total, "ufm_match_topk: workspace of %lld bytes, %lld needed", (long long)ws_bytes, m.total);
    const hipStream_t st = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)ws;
    unsigned long long* ping = keys + m.keys_bytes / 8;
    unsigned long long* pong = ping + m.list_bytes / 8;
    hipLaunchKernelGGL(match_chunk_sort_kernel, dim3(m.nchunks, B), dim3(SORT_THREADS), 0, st, keys, m.ncells, m.nchunks, m.L, ping);
    UFM_CHECK_LAUNCH("ufm_match_topk (chunk sort)");
    for (int n = m.nchunks; n > 1; n = (n + 1) / 2) {
        const int nout = (n + 1) / 2;
        hipLaunchKernelGGL(match_merge_kernel, dim3(nout, B), dim3(SORT_THREADS), 0, st, ping, n, m.L, pong, nout);
        UFM_CHECK_LAUNCH("ufm_match_topk (merge)");
        unsigned long long* tmp = ping;
        ping = pong, pong = tmp;
    }
    hipLaunchKernelGGL(match_write_kernel, dim3(B), dim3(256), 0, st, ping, m.L, K, flow_st, Hs, Ws, matches, scores, counts);
    UFM_CHECK_LAUNCH("ufm_match_topk (write)");
    return UFM_OK;
}
