// bz_net_tower_fp8_body.h -- the fused fp8 net kernel: f8::k_tower_fp8 and f8::k_sym_fp8 (inside namespace f8).
// Included twice by bz_net.hip, inside its anonymous namespace: with BZ_NET_SYM 0 it defines the plain kernel, with
// BZ_NET_SYM 1 the form that evaluates every position under a board symmetry (bz_sym.h): the bitboards
// are transformed in registers right after they are loaded and the policy row is stored through the inverse cell
// permutation.  One text, two kernels -- not a shared inlined body: the plain kernel then compiles to the very
// instructions it had before the symmetric form existed (a wrapper around a force-inlined template body moved their
// register allocation), and the resource tests find one kernel per name.

// 74.8 KB of LDS per workgroup: two workgroups per CU hide each other's epilogues (launch bound 2 waves per SIMD)
#if BZ_NET_SYM
__global__ void __launch_bounds__(256, 2) k_sym_fp8(TowerArgs T, bz_sym::Args Y) {
#else
__global__ void __launch_bounds__(256, 2) k_tower_fp8(TowerArgs T) {
#endif
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pos0 = blockIdx.x * 4;
    if (T.n_dev) { const int cnt = (int)*T.n_dev; T.n = cnt < T.n ? cnt : T.n; }  // clamped to the launch's rows (a count >= 2^31: negative, nothing runs)
    if (pos0 >= T.n) return;
    [[maybe_unused]] unsigned long long tacc[4] = {0, 0, 0, 0}, tk0 = 0, tk1 = 0, tr0 = 0, tr1 = 0;
    BZ_STAMP(tk0);
#ifdef BZ_EXP_STAMPS
    tr0 = __builtin_amdgcn_s_memrealtime();
#endif
    char* bufX = smem;
    char* bufM = smem + kBuf;
    const int r = lane & 31, h = lane >> 5;

    for (int i = tid; i < 2 * 4 * 9 * 8; i += 256) {  // zero cells 0, 9, .., 72 of 2 buffers x 4 positions (8 x 16 B each)
        int k = i & 7, j = (i >> 3) % 9, pb = i / 72;
        *reinterpret_cast<uint4*>(smem + pb * kTile + j * kRowC * kCell + k * 16) = make_uint4(0, 0, 0, 0);
    }
    // weight stream: tap t, k-step ks, co-tile w, 16-byte halves: wf8[(((t*2 + ks)*4 + w)*2 + half)*64 + lane]
    const uint4* ap = T.wf8 + (size_t)(w * 2) * 64;  // wave-uniform base + lane (SGPR-base addressing)
    v8i A0[2], A1[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        uint4 lo = ap[((ks * 4) * 2 + 0) * 64 + (unsigned)lane], hi = ap[((ks * 4) * 2 + 1) * 64 + (unsigned)lane];
        v8i v = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        A0[ks] = v;
    }
    ap += 2 * 4 * 2 * 64;

    // ---- stem (bf16 MFMA, exact 0/1 inputs) -> e4m3 activations
    {
        f32x16 acc[8];
        Scale sc;
        load_scale(sc, T.ones, T.stem_b, w, h);
        bf16x8 sa[2];
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) sa[kc] = __builtin_bit_cast(bf16x8, T.stem_wf[(kc * 4 + w) * 64 + lane]);
        int pos = pos0 + (r >> 3) < T.n ? pos0 + (r >> 3) : T.n - 1;  // every lane feeds ONE position in all units
        u64 own = T.own[pos], opp = T.opp[pos];
#if BZ_NET_SYM
        {
            const u32 s = bz_sym::of(Y, own, opp);
            own = bz_sym::board(own, Y.size, s); opp = bz_sym::board(opp, Y.size, s);
        }
#endif
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const unsigned n_own = nbhd(own, 8 * u + (r & 7)), n_opp = nbhd(opp, 8 * u + (r & 7));
            acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sa[0], stem_frag<0>(n_own, n_opp, h), (f32x16)(0.0f), 0, 0, 0);
            acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sa[1], stem_frag<1>(n_own, n_opp, h), acc[u], 0, 0, 0);
        }
        epilogue(acc, bufX, false, sc, w, r, h);
    }
    __syncthreads();

#pragma unroll 1
    for (int blk = 0; blk < T.n_layers / 2; ++blk) {
        conv_layer<0>(bufX, bufM, false, T.dq8 + (size_t)(2 * blk) * kTC, T.bias + (size_t)(2 * blk) * kTC, A0, A1, ap, w, r, h, tacc);
        conv_layer<1>(bufM, bufX, true, T.dq8 + (size_t)(2 * blk + 1) * kTC, T.bias + (size_t)(2 * blk + 1) * kTC, A0, A1, ap, w,
                      r, h, tacc);
    }

    BZ_STAMP(tk1);
    // ---- heads: wave p serves position p (conv1x1 in fp8, FCs in fp32)
    if (pos0 + w < T.n) {
        const int p = w, pos = pos0 + w;
#if BZ_NET_SYM
        const int dst = bz_sym::tau_inv(Y.size, bz_sym::of(Y, T.own[pos], T.opp[pos]), lane);
#else
        const int dst = lane;
#endif
        float* S = reinterpret_cast<float*>(bufM + p * 1024);
        const float pb0 = T.pol_b[0], pb1 = T.pol_b[1], vb = T.val_b[0];
        const float d0 = T.head_dq8[0], d1 = T.head_dq8[1], d2 = T.head_dq8[2];
        v8i hw[2];  // both head-conv fragments in flight before the first MFMA
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 lo = T.head_wf8[(ks * 2 + 0) * 64 + lane], hi = T.head_wf8[(ks * 2 + 1) * 64 + lane];
            v8i a = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            hw[ks] = a;
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            f32x16 acc = (f32x16)(0.0f);
            const int cell = 32 * nt + r;
            const int cb = cell_at(cell >> 3, cell & 7) + (((2 * h) ^ sw3(p, cell & 7)) << 4);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                v8i b = ld32(bufX + p * kTile, cb ^ (ks << 6), 0);
                acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(hw[ks], b, acc, 0, 0, 0, kUnit, 0, kUnit);
            }
            if (h == 0) {
                float a0 = acc[0] * d0 + pb0, a1 = acc[1] * d1 + pb1, a2 = acc[2] * d2 + vb;
                S[cell] = relu_f32(a0);
                S[64 + cell] = relu_f32(a1);
                S[128 + cell] = relu_f32(a2);
            }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        // (the fma chains below keep their order; the unroll factors only decide how many weight loads are in flight)
        float acc = T.polfc_b[lane], part = 0.0f;
#pragma unroll 8
        for (int i = 0; i < 128; i += 4) {
            f32x4 s4 = *reinterpret_cast<const f32x4*>(S + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_fmaf(s4[j], T.polfc_wT[(i + j) * 65 + lane], acc);
        }
        part = S[lane] * T.polfc_wT[lane * 65 + 64] + S[lane + 64] * T.polfc_wT[(lane + 64) * 65 + 64];
        part = wave_sum(part);
        T.logits[(size_t)pos * 65 + dst] = acc;
        if (lane == 0) T.logits[(size_t)pos * 65 + 64] = part + T.polfc_b[64];
        float vh = 0.0f;
        if (lane < T.VH) {
            float a = T.v1_b[lane];
#pragma unroll 32
            for (int i = 0; i < 64; ++i) a = __builtin_fmaf(S[128 + i], T.v1_wT[i * T.VH + lane], a);
            vh = relu_f32(a) * T.v2_w[lane];
        }
        vh = wave_sum(vh);
        if (lane == 0) T.value[pos] = tanhf_spec(vh + T.v2_b[0]);
    }
#ifdef BZ_EXP_STAMPS
    unsigned long long tk2; BZ_STAMP(tk2);
    tr1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0 && blockIdx.x < 4096) {
        unsigned long long* d = g_dbg + blockIdx.x * 8;
        d[0] = tacc[0]; d[1] = tacc[1]; d[2] = tacc[2]; d[3] = tk1 - tk0; d[4] = tk2 - tk0; d[5] = tr1 - tr0; d[6] = tk0; d[7] = tr0;
    }
#endif
}
