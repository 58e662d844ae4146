// bz_net_ends_body.h -- the two ends of the f32 parity path: k_stem / k_heads and k_sym_stem / k_sym_heads.
// Included twice by bz_net.hip, inside its anonymous namespace: with BZ_NET_SYM 0 it defines the plain kernels, with
// BZ_NET_SYM 1 the form that evaluates every position under a board symmetry (bz_sym.h): the bitboards
// are transformed in registers right after they are loaded and the policy row is stored through the inverse cell
// permutation.  One text, two kernels -- not a shared inlined body: the plain kernels then compile to the very
// instructions they had before the symmetric form existed (a wrapper around a force-inlined template body moved their
// register allocation), and the resource tests find one kernel per name.

// ------------------------------------------------------------------ stem
// thread = output channel, block = position.  x in {0,1}: fmaf(1,w,acc) == acc + w.
template <class OutT>
#if BZ_NET_SYM
__global__ void k_sym_stem(const u64* __restrict__ own, const u64* __restrict__ opp, int n, const u32* n_dev, int C,
                           const float* __restrict__ w, const float* __restrict__ b, OutT* __restrict__ out, bz_sym::Args Y) {
#else
__global__ void k_stem(const u64* __restrict__ own, const u64* __restrict__ opp, int n, const u32* n_dev, int C,
                       const float* __restrict__ w, const float* __restrict__ b, OutT* __restrict__ out) {
#endif
    int pos = blockIdx.x, co = threadIdx.x;
    if (n_dev) n = (int)*n_dev;
    if (pos >= n || co >= C) return;
    u64 me = own[pos], you = opp[pos];
#if BZ_NET_SYM
    {
        const u32 s = bz_sym::of(Y, me, you);
        me = bz_sym::board(me, Y.size, s); you = bz_sym::board(you, Y.size, s);
    }
#endif
    float wr[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) wr[i] = w[i * C + co];
    float bias = b[co];
    for (int cell = 0; cell < 64; ++cell) {
        int y = cell >> 3, x = cell & 7;
        float acc = bias;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            if (yy < 0 || yy > 7 || xx < 0 || xx > 7) continue;
            int c2 = yy * 8 + xx;
            // the oracle's fmaf(plane, w, acc) with the plane in {0, 1}: a stone adds w, an empty cell adds 0 * w (NaN for
            // an infinite w, as torch's convolution gives)
            acc = __builtin_fmaf((float)((me >> c2) & 1ULL), wr[2 * t], acc);
            acc = __builtin_fmaf((float)((you >> c2) & 1ULL), wr[2 * t + 1], acc);
        }
        out[((size_t)pos * 64 + cell) * C + co] = (OutT)relu_f32(acc);
    }
}

// ------------------------------------------------------------------ heads (both paths)
// block = position, 192 threads.  Every dot product is a sequential fmaf chain in
// the oracle's order, so with f32 activations the result is bit-identical.
template <class InT>
#if BZ_NET_SYM
__global__ void __launch_bounds__(192) k_sym_heads(const InT* __restrict__ act, int n, const u32* n_dev, int C, int VH,
                                                   const float* __restrict__ pol_w, const float* __restrict__ pol_b,
                                                   const float* __restrict__ polfc_wT, const float* __restrict__ polfc_b,
                                                   const float* __restrict__ val_w, const float* __restrict__ val_b,
                                                   const float* __restrict__ v1_wT, const float* __restrict__ v1_b,
                                                   const float* __restrict__ v2_w, const float* __restrict__ v2_b,
                                                   float* __restrict__ logits, float* __restrict__ value,
                                                   const u64* __restrict__ own, const u64* __restrict__ opp, bz_sym::Args Y) {
#else
__global__ void __launch_bounds__(192) k_heads(const InT* __restrict__ act, int n, const u32* n_dev, int C, int VH,
                                               const float* __restrict__ pol_w, const float* __restrict__ pol_b,
                                               const float* __restrict__ polfc_wT, const float* __restrict__ polfc_b,
                                               const float* __restrict__ val_w, const float* __restrict__ val_b,
                                               const float* __restrict__ v1_wT, const float* __restrict__ v1_b,
                                               const float* __restrict__ v2_w, const float* __restrict__ v2_b,
                                               float* __restrict__ logits, float* __restrict__ value) {
#endif
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* xs = reinterpret_cast<float*>(smem_raw);  // [64][C+1]
    float* pf = xs + 64 * (C + 1);                   // [128]
    float* vf = pf + 128;                            // [64]
    float* vh = vf + 64;                             // [VH]
    int pos = blockIdx.x, tid = threadIdx.x;
    if (n_dev) n = (int)*n_dev;
    if (pos >= n) return;
    const InT* x = act + (size_t)pos * 64 * C;
    for (int i = tid; i < 64 * C; i += 192) xs[(i / C) * (C + 1) + (i % C)] = (float)x[i];
    __syncthreads();
    {   // conv1x1: threads 0..127 -> policy (j, cell); 128..191 -> value (cell)
        int cell = tid & 63, j = tid >> 6;
        const float* wj = j < 2 ? pol_w + (size_t)j * C : val_w;
        float acc = j < 2 ? pol_b[j] : val_b[0];
        const float* xi = xs + cell * (C + 1);
        for (int c = 0; c < C; ++c) acc = __builtin_fmaf(xi[c], wj[c], acc);
        acc = relu_f32(acc);
        if (j < 2) pf[j * 64 + cell] = acc; else vf[cell] = acc;
    }
    __syncthreads();
    if (tid < 65) {
        float acc = polfc_b[tid];
        for (int i = 0; i < 128; ++i) acc = __builtin_fmaf(pf[i], polfc_wT[i * 65 + tid], acc);
#if BZ_NET_SYM  // logit a of the transformed position belongs to the cell that T_s moved onto a
        logits[(size_t)pos * 65 + bz_sym::tau_inv(Y.size, bz_sym::of(Y, own[pos], opp[pos]), tid)] = acc;
#else
        logits[(size_t)pos * 65 + tid] = acc;
#endif
    } else if (tid >= 128 && tid - 128 < VH) {
        int h = tid - 128;
        float acc = v1_b[h];
        for (int i = 0; i < 64; ++i) acc = __builtin_fmaf(vf[i], v1_wT[i * VH + h], acc);
        vh[h] = relu_f32(acc);
    }
    __syncthreads();
    if (tid == 0) {
        float acc = v2_b[0];
        for (int h = 0; h < VH; ++h) acc = __builtin_fmaf(vh[h], v2_w[h], acc);
        value[pos] = tanhf_spec(acc);
    }
}
