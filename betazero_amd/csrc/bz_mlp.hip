// bz_mlp.hip -- the reference's tic-tac-toe policy MLP (SL/neural_networks.py: Linear(9,H)-ReLU-Linear(H,H)-ReLU-
// Linear(H,H)-ReLU-Linear(H,9), logits only) on gfx950: forward in an fp32 parity mode and a bf16 MFMA mode, and the
// supervised training step of SL/train.py (softmax cross-entropy on the argmax target, Adam).  DESIGN.md 11.
// The same net with a value head (TicTacToePVNet: fc4 has a tenth row, v = tanh of it) goes through the same kernels with
// NO = 10 outputs, and has a training step of its own (soft policy targets, a value loss).
//
// Weight forms kept in the workspace (written by bz_mlp_create / bz_mlp_update, and by the training step's Adam kernel):
//  - wT: fp32, every weight matrix transposed ([in][out], out contiguous) so that the f32 kernels' lanes -- one per
//    output unit -- read consecutive words; biases as they are.  Same element count as the torch vector.
//  - frag: bf16 fragments of v_mfma_f32_16x16x32_bf16 in the order the bf16 kernel reads them (one uint4 per lane).
//    Rebuilt on the device from wT (k_mlp_pack_bf16) whenever wT changed since the last bf16 forward.
#include <math.h>
#include <new>
#include <string.h>
#include <vector>

#include "bz_common.h"
#include "bz_math.h"

using namespace bz;

namespace {
typedef __attribute__((ext_vector_type(8))) __bf16 m_bf16x8;
typedef __attribute__((ext_vector_type(4))) float m_f32x4;

constexpr int kIn = 9, kOut = 9, kOutPV = 10;
constexpr int kF32Rows = 16;   // positions per workgroup of the f32 forward
constexpr int kTrainRows = 4;  // ... of the training step's forward/backward kernel (batch 128 -> 32 workgroups)
constexpr int kThreads = 256;

inline bool h_ok(int H) { return H >= 32 && H <= 512 && H % 32 == 0; }

// flat torch order: fc1.w[H][9] fc1.b[H] fc2.w[H][H] fc2.b[H] fc3.w[H][H] fc3.b[H] fc4.w[NO][H] fc4.b[NO]
// NO = 9 (TicTacToeNet, policy only) or 10 (TicTacToePVNet: row 9 of fc4 is the value pre-activation u, v = tanh(u))
struct Layout {
    int64_t w[4], b[4], total;
    int K[4], N[4];
    __host__ __device__ Layout(int H, int NO) {
        const int Ks[4] = {kIn, H, H, H}, Ns[4] = {H, H, H, NO};
        int64_t o = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            K[l] = Ks[l]; N[l] = Ns[l];
            w[l] = o; o += (int64_t)Ks[l] * Ns[l];
            b[l] = o; o += Ns[l];
        }
        total = o;
    }
};

// bf16 fragments: layer l has JT(l) output tiles of 16 and KB(l) k-blocks of 32; fragment (jt, kb) = 64 lanes x 8 bf16
__host__ __device__ inline int frag_jt(int l, int H) { return l == 3 ? 1 : H / 16; }
__host__ __device__ inline int frag_kb(int l, int H) { return l == 0 ? 1 : H / 32; }
__host__ __device__ inline int64_t frag_off(int l, int H) {  // in uint4 units
    int64_t o = 0;
    for (int i = 0; i < l; ++i) o += (int64_t)frag_jt(i, H) * frag_kb(i, H) * 64;
    return o;
}
// the k a fragment slot stands for.  Layer 0 reads the 9 inputs as k = 8q + i.  Layers 1..3 read the previous layer's
// accumulators in place: tile 2kb of them holds units 32kb + 4q + i (i < 4) on lane group q, tile 2kb + 1 units
// 32kb + 16 + 4q + i -- so slot i of lane group q in k-block kb is unit 32kb + 4q + i (i < 4) or 32kb + 16 + 4q + i - 4.
__host__ __device__ inline int frag_k(int l, int kb, int q, int i) {
    if (l == 0) return 8 * q + i;
    return 32 * kb + (i < 4 ? 4 * q + i : 16 + 4 * q + i - 4);
}
}  // namespace

struct bz_mlp {
    int H, max_batch, NO;
    float* wT;      // device, Layout(H).total floats
    uint4* frag;    // device, bf16 fragments
    bool frag_stale;
};

namespace {
struct MlpNeed {
    int64_t wT, frag, total;
    MlpNeed(int H, int NO) {
        Layout L(H, NO);
        wT = 0;
        frag = (L.total * 4 + 255) & ~int64_t(255);
        total = frag + frag_off(4, H) * 16;
    }
};

// ---- input: row r, cell k -> x (bitboards: own_k - opp_k; states: x[r][k] as given)
struct MlpIn {
    const uint64_t* own; const uint64_t* opp; const float* x;
    __device__ __forceinline__ float at(int r, int k) const {
        if (x) return x[(size_t)r * kIn + k];
        return (float)((int)((own[r] >> k) & 1ull) - (int)((opp[r] >> k) & 1ull));
    }
};
__device__ __forceinline__ int row_count(int max_n, const uint32_t* n_dev) {
    if (!n_dev) return max_n;
    const int c = (int)*n_dev;
    return c < max_n ? c : max_n;
}

// ---- f32: one layer for R rows held in LDS as [k][R] (R contiguous).  Lane j of the workgroup owns output units
// j, j + 256: y = sum over k = 0, 1, ..., K-1 of fmaf(wT[k][j], in[k][r], .) from 0, then + b[j] (then ReLU).  This order
// is the documented one: run to run, and batch to batch, a row's result is the same bits.
template <int R>
__device__ __forceinline__ void f32_layer(const float* __restrict__ wT, const float* __restrict__ b, int K, int N,
                                          const float* in, float* out, bool relu) {
    for (int j = threadIdx.x; j < N; j += kThreads) {
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float w = wT[(size_t)k * N + j];
#pragma unroll
            for (int r4 = 0; r4 < R; r4 += 4) {
                const float4 a = *reinterpret_cast<const float4*>(in + k * R + r4);
                acc[r4] = fmaf(w, a.x, acc[r4]); acc[r4 + 1] = fmaf(w, a.y, acc[r4 + 1]);
                acc[r4 + 2] = fmaf(w, a.z, acc[r4 + 2]); acc[r4 + 3] = fmaf(w, a.w, acc[r4 + 3]);
            }
        }
        const float bj = b[j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float y = acc[r] + bj;
            out[j * R + r] = relu && y < 0.0f ? 0.0f : y;  // torch's ReLU: a NaN passes (fmaxf would make it 0)
        }
    }
}

__global__ void __launch_bounds__(kThreads) k_mlp_f32(const float* __restrict__ wT, int H, int NO, MlpIn in, int max_n,
                                                      const uint32_t* n_dev, float* __restrict__ logits, float* __restrict__ value) {
    extern __shared__ float4 s_dyn4[];
    float* bufA = reinterpret_cast<float*>(s_dyn4);
    float* bufB = bufA + (size_t)H * kF32Rows;
    constexpr int R = kF32Rows;
    const int cnt = row_count(max_n, n_dev);
    const int r0 = blockIdx.x * R;
    if (r0 >= cnt) return;
    const Layout L(H, NO);
    for (int t = threadIdx.x; t < kIn * R; t += kThreads) {
        const int k = t / R, r = t % R;
        bufB[t] = r0 + r < cnt ? in.at(r0 + r, k) : 0.0f;
    }
    __syncthreads();
    f32_layer<R>(wT + L.w[0], wT + L.b[0], kIn, H, bufB, bufA, true); __syncthreads();
    f32_layer<R>(wT + L.w[1], wT + L.b[1], H, H, bufA, bufB, true); __syncthreads();
    f32_layer<R>(wT + L.w[2], wT + L.b[2], H, H, bufB, bufA, true); __syncthreads();
    f32_layer<R>(wT + L.w[3], wT + L.b[3], H, NO, bufA, bufB, false); __syncthreads();
    for (int t = threadIdx.x; t < kOut * R; t += kThreads) {
        const int r = t / kOut, o = t % kOut;
        if (r0 + r < cnt) logits[(size_t)(r0 + r) * kOut + o] = bufB[o * R + r];
    }
    // unit 9 of a PV net went through the same chain as the logits: v = tanh(u); a policy-only net has no value, 0
    if (value && threadIdx.x < R && r0 + (int)threadIdx.x < cnt)
        value[r0 + threadIdx.x] = NO > kOut ? tanhf_spec(bufB[kOut * R + threadIdx.x]) : 0.0f;
}

// ---- bf16: one wave per 16 positions, every layer as out^T = W . act^T on v_mfma_f32_16x16x32_bf16 (A = weights,
// row = output unit; B = activations, column = position).  The accumulators of layer l are, after bias + ReLU + the
// bf16 rounding, the B operand of layer l + 1 as they lie (frag_k); activations never leave the registers.
template <int H>
__global__ void __launch_bounds__(64) k_mlp_bf16(const uint4* __restrict__ frag, const float* __restrict__ wT, int NO, MlpIn in,
                                                 int max_n, const uint32_t* n_dev, float* __restrict__ logits,
                                                 float* __restrict__ value) {
    constexpr int KB = H / 32;
    const int lane = threadIdx.x, col = lane & 15, q = lane >> 4;
    const int cnt = row_count(max_n, n_dev);
    const int r = blockIdx.x * 16 + col;
    if (blockIdx.x * 16 >= cnt) return;
    const bool ok = r < cnt;
    const Layout L(H, NO);
    m_bf16x8 x0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = 8 * q + i;
        x0[i] = (__bf16)((ok && k < kIn) ? in.at(r, k) : 0.0f);
    }
    m_bf16x8 act[KB], nxt[KB];
    // layer 0: K = 9 (one k-block), H outputs
    {
        const uint4* f = frag + frag_off(0, H);
        const float* b = wT + L.b[0];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            m_f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
            const uint4 a0 = f[(size_t)(2 * kb) * 64 + lane], a1 = f[(size_t)(2 * kb + 1) * 64 + lane];
            c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(m_bf16x8, a0), x0, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(m_bf16x8, a1), x0, c1, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                act[kb][i] = (__bf16)fmaxf(c0[i] + b[32 * kb + 4 * q + i], 0.0f);
                act[kb][4 + i] = (__bf16)fmaxf(c1[i] + b[32 * kb + 16 + 4 * q + i], 0.0f);
            }
        }
    }
    // layers 1 and 2: H x H
#pragma unroll
    for (int l = 1; l <= 2; ++l) {
        const uint4* f = frag + frag_off(l, H);
        const float* b = wT + L.b[l];
#pragma unroll
        for (int ob = 0; ob < KB; ++ob) {  // output tiles 2ob, 2ob + 1 = the next layer's k-block ob
            m_f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                const uint4 a0 = f[((size_t)(2 * ob) * KB + kb) * 64 + lane];
                const uint4 a1 = f[((size_t)(2 * ob + 1) * KB + kb) * 64 + lane];
                c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(m_bf16x8, a0), act[kb], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(m_bf16x8, a1), act[kb], c1, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                nxt[ob][i] = (__bf16)fmaxf(c0[i] + b[32 * ob + 4 * q + i], 0.0f);
                nxt[ob][4 + i] = (__bf16)fmaxf(c1[i] + b[32 * ob + 16 + 4 * q + i], 0.0f);
            }
        }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) act[kb] = nxt[kb];
    }
    // layer 3: NO outputs (one tile of 16, rows NO..15 zero weights); row 9 of a PV net is the value pre-activation, which
    // the MFMA leaves in c[1] of lane group 2
    {
        const uint4* f = frag + frag_off(3, H);
        m_f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(m_bf16x8, f[(size_t)kb * 64 + lane]), act[kb], c, 0, 0, 0);
        if (ok) {
            const float* b = wT + L.b[3];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = 4 * q + i;
                if (o < kOut) logits[(size_t)r * kOut + o] = c[i] + b[o];
            }
            if (value) {
                if (NO > kOut) { if (q == 2) value[r] = tanhf_spec(c[1] + b[kOut]); }
                else if (q == 0) value[r] = 0.0f;
            }
        }
    }
}

// wT (fp32, [in][out]) -> bf16 fragments; one thread per (fragment, lane)
__global__ void k_mlp_pack_bf16(const float* __restrict__ wT, int H, int NO, uint4* __restrict__ frag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= frag_off(4, H)) return;
    const int l = t >= frag_off(3, H) ? 3 : (t >= frag_off(2, H) ? 2 : (t >= frag_off(1, H) ? 1 : 0));
    const Layout L(H, NO);
    const int K = l == 0 ? kIn : H, N = l == 3 ? NO : H;
    const int64_t w0 = l == 0 ? L.w[0] : (l == 1 ? L.w[1] : (l == 2 ? L.w[2] : L.w[3]));
    const int64_t u = t - frag_off(l, H);
    const int lane = (int)(u % 64), fidx = (int)(u / 64);
    const int KB = frag_kb(l, H), jt = fidx / KB, kb = fidx % KB;
    const int j = jt * 16 + (lane & 15), q = lane >> 4;
    m_bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = frag_k(l, kb, q, i);
        const bool in = j < N && k < K;
        v[i] = (__bf16)(in ? wT[w0 + (int64_t)k * N + j] : 0.0f);
    }
    frag[t] = __builtin_bit_cast(uint4, v);
}

int32_t pack_bf16(bz_mlp* m, hipStream_t s) {
    const int64_t n = frag_off(4, m->H);
    hipLaunchKernelGGL(k_mlp_pack_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, m->wT, m->H, m->NO, m->frag);
    BZ_LAUNCH_CHECK("k_mlp_pack_bf16");
    m->frag_stale = false;
    return BZ_OK;
}

// torch layout (host) -> wT (host), then upload and rebuild the fragments
int32_t upload(bz_mlp* m, const float* p, hipStream_t s) {
    const Layout L(m->H, m->NO);
    std::vector<float> t((size_t)L.total);
    for (int l = 0; l < 4; ++l) {
        const int K = L.K[l], N = L.N[l];
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < K; ++k) t[(size_t)(L.w[l] + (int64_t)k * N + j)] = p[L.w[l] + (int64_t)j * K + k];
        memcpy(&t[(size_t)L.b[l]], p + L.b[l], (size_t)N * 4);
    }
    BZ_HIP(hipMemcpyAsync(m->wT, t.data(), (size_t)L.total * 4, hipMemcpyHostToDevice, s));
    int32_t rc = pack_bf16(m, s);
    if (rc != BZ_OK) return rc;
    BZ_HIP(hipStreamSynchronize(s));  // the host staging vector dies here
    return BZ_OK;
}
}  // namespace

namespace {
int32_t create(const char* who, int32_t H, int NO, int32_t max_batch, const float* params_host, void* ws, int64_t bytes, void* stream,
               bz_mlp** out) {
    if (!(h_ok(H) && max_batch >= 1)) { set_error("%s: H must be a multiple of 32 in 32..512, max_batch >= 1", who); return BZ_EINVAL; }
    if (!(params_host && ws && out)) { set_error("%s: null pointer", who); return BZ_EINVAL; }
    const MlpNeed need(H, NO);
    if (bytes < need.total) { set_error("%s: workspace too small (%lld < %lld)", who, (long long)bytes, (long long)need.total); return BZ_ENOMEM; }
    if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) { set_error("%s: workspace must be 256-byte aligned", who); return BZ_EINVAL; }
    if (bz_device_count() <= 0) { set_error("%s: no HIP device (the MLP has no CPU path)", who); return BZ_ENOGPU; }
    bz_mlp* m = new (std::nothrow) bz_mlp();
    if (!m) { set_error("out of host memory"); return BZ_ENOMEM; }
    m->H = H; m->max_batch = max_batch; m->NO = NO;
    m->wT = reinterpret_cast<float*>(static_cast<char*>(ws) + need.wT);
    m->frag = reinterpret_cast<uint4*>(static_cast<char*>(ws) + need.frag);
    int32_t rc = upload(m, params_host, (hipStream_t)stream);
    if (rc != BZ_OK) { delete m; return rc; }
    if (H * kF32Rows * 2 * 4 > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_mlp_f32), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           H * kF32Rows * 2 * 4);
        if (e != hipSuccess) { delete m; return hip_fail(e, "hipFuncSetAttribute(k_mlp_f32)"); }
    }
    *out = m;
    return BZ_OK;
}
}  // namespace

BZ_EXPORT int64_t bz_mlp_param_count(int32_t H) {
    if (!h_ok(H)) { set_error("bz_mlp_param_count: H must be a multiple of 32 in 32..512"); return -1; }
    return Layout(H, kOut).total;
}

BZ_EXPORT int64_t bz_mlp_pv_param_count(int32_t H) {
    if (!h_ok(H)) { set_error("bz_mlp_pv_param_count: H must be a multiple of 32 in 32..512"); return -1; }
    return Layout(H, kOutPV).total;
}

BZ_EXPORT int64_t bz_mlp_workspace_bytes(int32_t H, int32_t max_batch) {
    if (!h_ok(H) || max_batch < 1) { set_error("bz_mlp_workspace_bytes: H must be a multiple of 32 in 32..512, max_batch >= 1"); return -1; }
    return MlpNeed(H, kOut).total;
}

BZ_EXPORT int64_t bz_mlp_pv_workspace_bytes(int32_t H, int32_t max_batch) {
    if (!h_ok(H) || max_batch < 1) { set_error("bz_mlp_pv_workspace_bytes: H must be a multiple of 32 in 32..512, max_batch >= 1"); return -1; }
    return MlpNeed(H, kOutPV).total;
}

BZ_EXPORT int32_t bz_mlp_create(int32_t H, int32_t max_batch, const float* params_host, void* ws, int64_t bytes, void* stream,
                                bz_mlp** out) {
    return create("bz_mlp_create", H, kOut, max_batch, params_host, ws, bytes, stream, out);
}

BZ_EXPORT int32_t bz_mlp_create_pv(int32_t H, int32_t max_batch, const float* params_host, void* ws, int64_t bytes, void* stream,
                                   bz_mlp** out) {
    return create("bz_mlp_create_pv", H, kOutPV, max_batch, params_host, ws, bytes, stream, out);
}

BZ_EXPORT int32_t bz_mlp_has_value(const bz_mlp* m) { return m && m->NO > kOut ? 1 : 0; }

BZ_EXPORT int32_t bz_mlp_destroy(bz_mlp* m) {
    delete m;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_mlp_update(bz_mlp* m, const float* params_host, void* stream) {
    BZ_REQUIRE(m && params_host, "bz_mlp_update: null pointer");
    // searches in flight on ANY stream must not see half-replaced weights: drain the device first
    BZ_HIP(hipDeviceSynchronize());
    return upload(m, params_host, (hipStream_t)stream);
}

int32_t bz_mlp_max_batch(const bz_mlp* m) { return m ? m->max_batch : 0; }

int32_t bz_mlp_forward_dev(bz_mlp* m, int bf16, const uint64_t* own, const uint64_t* opp, const float* x, int32_t max_n,
                           const uint32_t* n_dev, float* logits, float* value, void* stream) {
    BZ_REQUIRE(m && logits && (x || (own && opp)), "bz_mlp_forward: null pointer");
    BZ_REQUIRE(max_n >= 0 && max_n <= m->max_batch, "bz_mlp_forward: n exceeds max_batch");
    if (max_n == 0) return BZ_OK;
    hipStream_t s = (hipStream_t)stream;
    MlpIn in; in.own = own; in.opp = opp; in.x = x;
    if (!bf16) {
        hipLaunchKernelGGL(k_mlp_f32, dim3((max_n + kF32Rows - 1) / kF32Rows), dim3(kThreads), (size_t)m->H * kF32Rows * 2 * 4, s,
                           m->wT, m->H, m->NO, in, max_n, n_dev, logits, value);
        BZ_LAUNCH_CHECK("k_mlp_f32");
        return BZ_OK;
    }
    if (m->frag_stale) {
        int32_t rc = pack_bf16(m, s);
        if (rc != BZ_OK) return rc;
    }
    const dim3 grid((max_n + 15) / 16);
    switch (m->H) {
#define BZ_MLP_H(HH) case HH: hipLaunchKernelGGL(k_mlp_bf16<HH>, grid, dim3(64), 0, s, m->frag, m->wT, m->NO, in, max_n, n_dev, logits, value); break;
        BZ_MLP_H(32) BZ_MLP_H(64) BZ_MLP_H(96) BZ_MLP_H(128) BZ_MLP_H(160) BZ_MLP_H(192) BZ_MLP_H(224) BZ_MLP_H(256)
        BZ_MLP_H(288) BZ_MLP_H(320) BZ_MLP_H(352) BZ_MLP_H(384) BZ_MLP_H(416) BZ_MLP_H(448) BZ_MLP_H(480) BZ_MLP_H(512)
#undef BZ_MLP_H
    default: set_error("bz_mlp_forward_bf16: bad H"); return BZ_EINVAL;
    }
    BZ_LAUNCH_CHECK("k_mlp_bf16");
    return BZ_OK;
}

BZ_EXPORT int32_t bz_mlp_forward_f32(bz_mlp* m, const uint64_t* own, const uint64_t* opp, int32_t n, float* logits, void* stream) {
    BZ_REQUIRE(own && opp, "bz_mlp_forward_f32: null pointer");
    return bz_mlp_forward_dev(m, 0, own, opp, nullptr, n, nullptr, logits, nullptr, stream);
}
BZ_EXPORT int32_t bz_mlp_forward_bf16(bz_mlp* m, const uint64_t* own, const uint64_t* opp, int32_t n, float* logits, void* stream) {
    BZ_REQUIRE(own && opp, "bz_mlp_forward_bf16: null pointer");
    return bz_mlp_forward_dev(m, 1, own, opp, nullptr, n, nullptr, logits, nullptr, stream);
}
BZ_EXPORT int32_t bz_mlp_forward_states_f32(bz_mlp* m, const float* x, int32_t n, float* logits, void* stream) {
    BZ_REQUIRE(x, "bz_mlp_forward_states_f32: null pointer");
    return bz_mlp_forward_dev(m, 0, nullptr, nullptr, x, n, nullptr, logits, nullptr, stream);
}
BZ_EXPORT int32_t bz_mlp_forward_states_bf16(bz_mlp* m, const float* x, int32_t n, float* logits, void* stream) {
    BZ_REQUIRE(x, "bz_mlp_forward_states_bf16: null pointer");
    return bz_mlp_forward_dev(m, 1, nullptr, nullptr, x, n, nullptr, logits, nullptr, stream);
}


// logits and value of a PV handle (bz_mlp_create_pv); a policy-only handle has no value to give
#define BZ_MLP_PV(who) \
    BZ_REQUIRE(m && value, who ": null pointer"); \
    BZ_REQUIRE(m->NO > kOut, who ": the net has no value head (bz_mlp_create_pv makes one that has)")
BZ_EXPORT int32_t bz_mlp_forward_pv_f32(bz_mlp* m, const uint64_t* own, const uint64_t* opp, int32_t n, float* logits, float* value,
                                        void* stream) {
    BZ_MLP_PV("bz_mlp_forward_pv_f32");
    BZ_REQUIRE(own && opp, "bz_mlp_forward_pv_f32: null pointer");
    return bz_mlp_forward_dev(m, 0, own, opp, nullptr, n, nullptr, logits, value, stream);
}
BZ_EXPORT int32_t bz_mlp_forward_pv_bf16(bz_mlp* m, const uint64_t* own, const uint64_t* opp, int32_t n, float* logits, float* value,
                                         void* stream) {
    BZ_MLP_PV("bz_mlp_forward_pv_bf16");
    BZ_REQUIRE(own && opp, "bz_mlp_forward_pv_bf16: null pointer");
    return bz_mlp_forward_dev(m, 1, own, opp, nullptr, n, nullptr, logits, value, stream);
}
BZ_EXPORT int32_t bz_mlp_forward_pv_states_f32(bz_mlp* m, const float* x, int32_t n, float* logits, float* value, void* stream) {
    BZ_MLP_PV("bz_mlp_forward_pv_states_f32");
    BZ_REQUIRE(x, "bz_mlp_forward_pv_states_f32: null pointer");
    return bz_mlp_forward_dev(m, 0, nullptr, nullptr, x, n, nullptr, logits, value, stream);
}
BZ_EXPORT int32_t bz_mlp_forward_pv_states_bf16(bz_mlp* m, const float* x, int32_t n, float* logits, float* value, void* stream) {
    BZ_MLP_PV("bz_mlp_forward_pv_states_bf16");
    BZ_REQUIRE(x, "bz_mlp_forward_pv_states_bf16: null pointer");
    return bz_mlp_forward_dev(m, 1, nullptr, nullptr, x, n, nullptr, logits, value, stream);
}
#undef BZ_MLP_PV

// ---------------------------------------------------------------------------------------------------------------------
// Training step (SL/train.py: CrossEntropyLoss(logits, argmax action), mean over the batch, then Adam).  Two launches:
//  1. k_mlp_train_fb: per kTrainRows rows -- the f32 forward (saving the post-ReLU activations), softmax-CE gradient,
//     backward-data through fc4..fc2 (ReLU masks from the saved activations); writes a1..a3, d1..d3, g4 and the rows' loss.
//  2. k_mlp_train_adam: one thread per parameter -- its gradient summed over the rows in ascending order (deterministic),
//     then Adam on (p, m, v) and the transposed copy the forward reads.  Block 0 also sums the loss (ascending rows).
// The PV step (k_mlp_train_fb_pv, bz_mlp_train_step_pv) is the same two launches on a PV net: soft policy targets pi and a
// value target vt per row, loss = sum_o pi_o (lse(z) - z_o) + c (v - vt)^2, fc4 and g4 ten outputs wide.
namespace {
struct TrainNeed {
    int64_t a[3], d[3], g4, rl, total;
    TrainNeed(int H, int B, int NO) {
        int64_t o = 0;
        auto take = [&](int64_t bytes) { int64_t r = o; o += (bytes + 255) & ~int64_t(255); return r; };
        for (int i = 0; i < 3; ++i) a[i] = take((int64_t)B * H * 4);
        for (int i = 0; i < 3; ++i) d[i] = take((int64_t)B * H * 4);
        g4 = take((int64_t)B * NO * 4);
        rl = take((int64_t)B * 4);
        total = o;
    }
};

struct TrainPtrs {
    float* a[3]; float* d[3]; float* g4; float* rl;
};

// d_in[r][k] = (sum over j ascending of fmaf(W[j][k], d_out[r][j])) * (a_in[r][k] > 0); W torch layout [N][K]
template <int R>
__device__ __forceinline__ void bwd_layer(const float* __restrict__ W, int K, int N, const float* dout_lds, const float* __restrict__ a_in,
                                          int r0, int cnt, float* din_lds, float* __restrict__ din_g) {
    for (int k = threadIdx.x; k < K; k += kThreads) {
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0f;
        for (int j = 0; j < N; ++j) {
            const float w = W[(size_t)j * K + k];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = fmaf(w, dout_lds[j * R + r], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float v = 0.0f;
            if (r0 + r < cnt && a_in[(size_t)(r0 + r) * K + k] > 0.0f) v = acc[r];
            din_lds[k * R + r] = v;
            if (r0 + r < cnt) din_g[(size_t)(r0 + r) * K + k] = v;
        }
    }
}

// what a row is trained towards: the supervised step's class index, or the PV step's (pi, vt) with the value weight c
struct TrainTarget {
    const int32_t* target;                   // [n], 0..8                         (NO = 9)
    const float* pi; const float* vt; float c;  // [n][9] >= 0, [n] in [-1, 1]    (NO = 10)
};

template <int NO>
__device__ __forceinline__ void train_fb(const float* __restrict__ wT, const float* __restrict__ p, int H, const float* __restrict__ x,
                                         const TrainTarget G, const float* __restrict__ row_w, int n, TrainPtrs T,
                                         float* __restrict__ logits_out, float* __restrict__ value_out, uint32_t* err) {
    constexpr int R = kTrainRows;
    extern __shared__ float4 s_dyn4[];
    float* bufA = reinterpret_cast<float*>(s_dyn4);
    float* bufB = bufA + (size_t)H * R;
    __shared__ float s_red[kThreads];
    const int r0 = blockIdx.x * R;
    const Layout L(H, NO);
    // sum of the row weights, in a fixed order (every workgroup computes the same bits)
    float sw = 0.0f;
    for (int r = threadIdx.x; r < n; r += kThreads) sw += row_w ? row_w[r] : 1.0f;
    s_red[threadIdx.x] = sw;
    for (int t = threadIdx.x; t < kIn * R; t += kThreads) {
        const int k = t / R, r = t % R;
        bufB[t] = r0 + r < n ? x[(size_t)(r0 + r) * kIn + k] : 0.0f;
    }
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_red[threadIdx.x] = s_red[threadIdx.x] + s_red[threadIdx.x + w];
        __syncthreads();
    }
    const float sumw = s_red[0];
    // forward; a_l saved as [row][unit] (the thread that writes unit j reads it back in the backward)
    const float* src = bufB;
    float* dst = bufA;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        f32_layer<R>(wT + L.w[l], wT + L.b[l], L.K[l], L.N[l], src, dst, l < 3);
        __syncthreads();
        if (l < 3)
            for (int j = threadIdx.x; j < H; j += kThreads)
                for (int r = 0; r < R; ++r)
                    if (r0 + r < n) T.a[l][(size_t)(r0 + r) * H + j] = dst[j * R + r];
        float* t = const_cast<float*>(src); src = dst; dst = t;
    }
    // src = fc4's outputs [NO][R]; the loss gradient on them, scaled by w_r / sum w
    float* g4l = dst;  // [NO][R]
    if ((int)threadIdx.x < R) {
        const int r = threadIdx.x, row = r0 + r;
        float g[NO];
        for (int o = 0; o < NO; ++o) g[o] = 0.0f;
        if (row < n) {
            const float w = row_w ? row_w[row] : 1.0f;
            float z[kOut], mx = -INFINITY;
            for (int o = 0; o < kOut; ++o) { z[o] = src[o * R + r]; mx = fmaxf(mx, z[o]); }
            if (logits_out)
                for (int o = 0; o < kOut; ++o) logits_out[(size_t)row * kOut + o] = z[o];
            float s = 0.0f;
            for (int o = 0; o < kOut; ++o) s += expf(z[o] - mx);
            const float scale = w / sumw;
            float loss = 0.0f;
            if (!(sumw > 0.0f)) atomicOr(err, 4u);
            if constexpr (NO == kOut) {
                const int t = G.target[row];
                if (t < 0 || t >= kOut) { if (w != 0.0f) atomicOr(err, 1u); }
                else if (w != 0.0f) {
                    const float ce = (mx + logf(s)) - z[t];
                    if (!isfinite(ce)) atomicOr(err, 2u);
                    loss = scale * ce;
                    for (int o = 0; o < kOut; ++o) g[o] = scale * (expf(z[o] - mx) / s - (o == t ? 1.0f : 0.0f));
                }
            } else {
                const float v = tanhf_spec(src[kOut * R + r]);  // the inference forward's value, bit for bit
                if (value_out) value_out[row] = v;
                if (w != 0.0f) {
                    float pi[kOut], sp = 0.0f;
                    bool bad = false;
                    for (int o = 0; o < kOut; ++o) {
                        pi[o] = G.pi[(size_t)row * kOut + o];
                        if (!(pi[o] >= 0.0f) || !isfinite(pi[o])) bad = true;
                        sp += pi[o];
                    }
                    const float vt = G.vt[row];
                    if (!(sp > 0.0f) || !(vt >= -1.0f && vt <= 1.0f)) bad = true;
                    if (bad) atomicOr(err, 1u);
                    else {
                        const float lse = mx + logf(s);
                        float ce = 0.0f;
                        for (int o = 0; o < kOut; ++o) ce += pi[o] * (lse - z[o]);
                        const float dv = v - vt;
                        const float rl = ce + G.c * (dv * dv);
                        if (!isfinite(rl)) atomicOr(err, 2u);
                        loss = scale * rl;
                        for (int o = 0; o < kOut; ++o) g[o] = scale * (sp * (expf(z[o] - mx) / s) - pi[o]);
                        g[kOut] = ((scale * G.c) * (2.0f * dv)) * (1.0f - v * v);
                    }
                }
            }
            T.rl[row] = loss;
            for (int o = 0; o < NO; ++o) T.g4[(size_t)row * NO + o] = g[o];
        }
        for (int o = 0; o < NO; ++o) g4l[o * R + r] = g[o];
    }
    __syncthreads();
    // backward-data: d3 = W4^T g4 * mask3, d2 = W3^T d3 * mask2, d1 = W2^T d2 * mask1
    float* other = const_cast<float*>(src);
    bwd_layer<R>(p + L.w[3], H, NO, g4l, T.a[2], r0, n, other, T.d[2]); __syncthreads();
    bwd_layer<R>(p + L.w[2], H, H, other, T.a[1], r0, n, g4l, T.d[1]); __syncthreads();
    bwd_layer<R>(p + L.w[1], H, H, g4l, T.a[0], r0, n, other, T.d[0]);
}

__global__ void __launch_bounds__(kThreads) k_mlp_train_fb(const float* __restrict__ wT, const float* __restrict__ p, int H,
                                                           const float* __restrict__ x, const int32_t* __restrict__ target,
                                                           const float* __restrict__ row_w, int n, TrainPtrs T,
                                                           float* __restrict__ logits_out, uint32_t* err) {
    TrainTarget G; G.target = target; G.pi = nullptr; G.vt = nullptr; G.c = 0.0f;
    train_fb<kOut>(wT, p, H, x, G, row_w, n, T, logits_out, nullptr, err);
}

__global__ void __launch_bounds__(kThreads) k_mlp_train_fb_pv(const float* __restrict__ wT, const float* __restrict__ p, int H,
                                                              const float* __restrict__ x, const float* __restrict__ pi,
                                                              const float* __restrict__ vt, float c, const float* __restrict__ row_w,
                                                              int n, TrainPtrs T, float* __restrict__ logits_out,
                                                              float* __restrict__ value_out, uint32_t* err) {
    TrainTarget G; G.target = nullptr; G.pi = pi; G.vt = vt; G.c = c;
    train_fb<kOutPV>(wT, p, H, x, G, row_w, n, T, logits_out, value_out, err);
}

struct AdamArgs { float lr, beta1, beta2, eps, step_size, bc2_sqrt; };

__global__ void __launch_bounds__(256) k_mlp_train_adam(int H, int NO, int n, const float* __restrict__ x, TrainPtrs T,
                                                        float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ grad, float* __restrict__ wT, AdamArgs A,
                                                        const uint32_t* __restrict__ err, float* __restrict__ loss) {
    const Layout L(H, NO);
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0 && loss) {
        float s = 0.0f;
        for (int r = 0; r < n; ++r) s += T.rl[r];
        *loss = s;
    }
    if (t >= L.total) return;
    const int l = t >= L.w[3] ? 3 : (t >= L.w[2] ? 2 : (t >= L.w[1] ? 1 : 0));
    const int K = l == 0 ? kIn : H, N = l == 3 ? NO : H;
    const int64_t wl = l == 0 ? L.w[0] : (l == 1 ? L.w[1] : (l == 2 ? L.w[2] : L.w[3]));
    const int64_t bl = wl + (int64_t)K * N;
    const float* dl = l == 3 ? T.g4 : (l == 2 ? T.d[2] : (l == 1 ? T.d[1] : T.d[0]));  // [n][N]
    const float* al = l == 0 ? x : (l == 1 ? T.a[0] : (l == 2 ? T.a[1] : T.a[2]));     // [n][K]
    float g = 0.0f;
    int64_t tw;  // index into wT
    if (t < bl) {
        const int64_t u = t - wl;
        const int j = (int)(u / K), k = (int)(u % K);
        for (int r = 0; r < n; ++r) g = fmaf(dl[(size_t)r * N + j], al[(size_t)r * K + k], g);
        tw = wl + (int64_t)k * N + j;
    } else {
        const int j = (int)(t - bl);
        for (int r = 0; r < n; ++r) g = g + dl[(size_t)r * N + j];
        tw = t;
    }
    if (grad) grad[t] = g;
    if (*err) return;  // a bad target / non-finite loss: the parameters stay as they were
    // torch.optim.Adam (no weight decay, not amsgrad): m.lerp_(g, 1 - beta1); v = v * beta2 + (1 - beta2) g g;
    // p -= step_size * m / (sqrt(v) / sqrt(bias_correction2) + eps)
    float mt = m[t], vt = v[t];
    mt = mt + (1.0f - A.beta1) * (g - mt);
    vt = vt * A.beta2 + (1.0f - A.beta2) * (g * g);
    const float denom = sqrtf(vt) / A.bc2_sqrt + A.eps;
    const float pt = p[t] - A.step_size * (mt / denom);
    m[t] = mt; v[t] = vt; p[t] = pt; wT[tw] = pt;
}

// the arguments both steps share, checked; then the workspace carved and the Adam scalars made
int32_t train_prepare(const char* who, const bz_mlp* mlp, int NO, int32_t n, const bz_mlp_adam* adam, void* ws, int64_t ws_bytes,
                      TrainPtrs* T, AdamArgs* A) {
    if (mlp->NO != NO) {
        set_error(NO == kOut ? "%s: the net has a value head (bz_mlp_train_step_pv trains it)"
                             : "%s: the net has no value head (bz_mlp_create_pv makes one that has)", who);
        return BZ_EINVAL;
    }
    if (!(n >= 1 && n <= mlp->max_batch)) { set_error("%s: need 1 <= n <= max_batch", who); return BZ_EINVAL; }
    if (!(adam->step >= 1 && adam->lr >= 0.0f && adam->beta1 >= 0.0f && adam->beta1 < 1.0f && adam->beta2 >= 0.0f &&
          adam->beta2 < 1.0f && adam->eps >= 0.0f)) { set_error("%s: bad Adam hyper-parameters", who); return BZ_EINVAL; }
    const TrainNeed need(mlp->H, n, NO);
    if (ws_bytes < need.total) { set_error("%s: workspace too small (bz_mlp_train_workspace_bytes)", who); return BZ_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) { set_error("%s: workspace must be 256-byte aligned", who); return BZ_EINVAL; }
    char* base = static_cast<char*>(ws);
    for (int i = 0; i < 3; ++i) { T->a[i] = reinterpret_cast<float*>(base + need.a[i]); T->d[i] = reinterpret_cast<float*>(base + need.d[i]); }
    T->g4 = reinterpret_cast<float*>(base + need.g4); T->rl = reinterpret_cast<float*>(base + need.rl);
    A->lr = adam->lr; A->beta1 = adam->beta1; A->beta2 = adam->beta2; A->eps = adam->eps;
    // torch computes the bias corrections in double on the host (capturable=False), then uses them as scalars
    const double bc1 = 1.0 - pow((double)adam->beta1, adam->step), bc2 = 1.0 - pow((double)adam->beta2, adam->step);
    A->step_size = (float)((double)adam->lr / bc1);
    A->bc2_sqrt = (float)sqrt(bc2);
    return BZ_OK;
}

int32_t train_adam(bz_mlp* mlp, int32_t n, const float* x, const TrainPtrs& T, float* params, float* m, float* v, float* grad,
                   const AdamArgs& A, const uint32_t* err, float* loss, hipStream_t s) {
    const int64_t P = Layout(mlp->H, mlp->NO).total;
    hipLaunchKernelGGL(k_mlp_train_adam, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, mlp->H, mlp->NO, n, x, T, params, m, v,
                       grad, mlp->wT, A, err, loss);
    BZ_LAUNCH_CHECK("k_mlp_train_adam");
    mlp->frag_stale = true;
    return BZ_OK;
}
}  // namespace

BZ_EXPORT int64_t bz_mlp_train_workspace_bytes(int32_t H, int32_t max_batch) {
    if (!h_ok(H) || max_batch < 1) { set_error("bz_mlp_train_workspace_bytes: H must be a multiple of 32 in 32..512, max_batch >= 1"); return -1; }
    return TrainNeed(H, max_batch, kOut).total;
}

BZ_EXPORT int64_t bz_mlp_train_pv_workspace_bytes(int32_t H, int32_t max_batch) {
    if (!h_ok(H) || max_batch < 1) { set_error("bz_mlp_train_pv_workspace_bytes: H must be a multiple of 32 in 32..512, max_batch >= 1"); return -1; }
    return TrainNeed(H, max_batch, kOutPV).total;
}

BZ_EXPORT int32_t bz_mlp_train_step(bz_mlp* mlp, float* params, float* m, float* v, float* grad, const float* x,
                                    const int32_t* target, const float* row_w, int32_t n, const bz_mlp_adam* adam,
                                    void* ws, int64_t ws_bytes, float* loss, float* logits, uint32_t* err, void* stream) {
    BZ_REQUIRE(mlp && params && m && v && x && target && adam && ws && err, "bz_mlp_train_step: null pointer");
    TrainPtrs T; AdamArgs A;
    int32_t rc = train_prepare("bz_mlp_train_step", mlp, kOut, n, adam, ws, ws_bytes, &T, &A);
    if (rc != BZ_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int H = mlp->H;
    {
        static unsigned done = 0;
        const int lds = H * kTrainRows * 2 * 4;
        hipError_t e = lds_attr_per_device(reinterpret_cast<const void*>(k_mlp_train_fb), lds, &done);
        if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_mlp_train_fb)");
        hipLaunchKernelGGL(k_mlp_train_fb, dim3((n + kTrainRows - 1) / kTrainRows), dim3(kThreads), (size_t)lds, s,
                           mlp->wT, params, H, x, target, row_w, n, T, logits, err);
        BZ_LAUNCH_CHECK("k_mlp_train_fb");
    }
    return train_adam(mlp, n, x, T, params, m, v, grad, A, err, loss, s);
}

BZ_EXPORT int32_t bz_mlp_train_step_pv(bz_mlp* mlp, float* params, float* m, float* v, float* grad, const float* x,
                                       const float* pi, const float* vt, const float* row_w, int32_t n, float value_weight,
                                       const bz_mlp_adam* adam, void* ws, int64_t ws_bytes, float* loss, float* logits, float* value,
                                       uint32_t* err, void* stream) {
    BZ_REQUIRE(mlp && params && m && v && x && pi && vt && adam && ws && err, "bz_mlp_train_step_pv: null pointer");
    BZ_REQUIRE(value_weight >= 0.0f && isfinite(value_weight), "bz_mlp_train_step_pv: value_weight must be finite and >= 0");
    TrainPtrs T; AdamArgs A;
    int32_t rc = train_prepare("bz_mlp_train_step_pv", mlp, kOutPV, n, adam, ws, ws_bytes, &T, &A);
    if (rc != BZ_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int H = mlp->H;
    {
        static unsigned done = 0;
        const int lds = H * kTrainRows * 2 * 4;
        hipError_t e = lds_attr_per_device(reinterpret_cast<const void*>(k_mlp_train_fb_pv), lds, &done);
        if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_mlp_train_fb_pv)");
        hipLaunchKernelGGL(k_mlp_train_fb_pv, dim3((n + kTrainRows - 1) / kTrainRows), dim3(kThreads), (size_t)lds, s,
                           mlp->wT, params, H, x, pi, vt, value_weight, row_w, n, T, logits, value, err);
        BZ_LAUNCH_CHECK("k_mlp_train_fb_pv");
    }
    return train_adam(mlp, n, x, T, params, m, v, grad, A, err, loss, s);
}
