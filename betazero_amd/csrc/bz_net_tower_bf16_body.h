// bz_net_tower_bf16_body.h -- the fused bf16 net kernel: k_tower_bf16<G>, k_sym_bf16<G> and k_edge_bf16<G>.
// Included three times by bz_net.hip, inside its anonymous namespace: with BZ_NET_SYM 0 it defines the plain kernel, with
// BZ_NET_SYM 1 the form that evaluates every position under a board symmetry (bz_sym.h): the bitboards
// are transformed in registers right after they are loaded and the policy row is stored through the inverse cell
// permutation; with BZ_NET_SYM 0 and BZ_NET_EDGE 1 the plain kernel again under a name of its own, for the geometry on
// the edge-aware cell tiling (Tw<128, 4, true, 1>, bz_tile_map.h).  One text, three kernels -- not a shared inlined body:
// the plain kernel then compiles to the very instructions it had before the other forms existed (a wrapper around a
// force-inlined template body moved their register allocation), and the resource tests find one kernel per name.

// The whole net forward for P positions per workgroup: stem (MFMA, K = 18 padded to 32, fed from
// the bitboards) -> residual tower (activations resident in LDS) -> heads (conv1x1 by MFMA, the
// small FCs by one wave per position).  HBM traffic per position: 16 B in, 264 B out.
template <class G>
__global__ void __launch_bounds__(256, 1)
#if BZ_NET_SYM
k_sym_bf16(TowerArgs T, bz_sym::Args Y) {  // (the name must not contain the plain kernel's: the resource tests look kernels up by substring)
#elif BZ_NET_EDGE
k_edge_bf16(TowerArgs T) {  // (likewise: neither of the other two names)
#else
k_tower_bf16(TowerArgs T) {
#endif
    constexpr int C = G::C, P = G::P, PW = G::PW, MW = G::MW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pos0 = blockIdx.x * P;
    // the [lo, hi] window sees the count as it stands (an adaptive pair's latency launch carries T.n = kAdaptT1: a larger
    // count is the other launch's); the rows are then clamped to the launch's own T.n, so that no count reaches past the
    // caller's buffers.  The window is one unsigned compare, which needs 0 <= lo <= hi (the host sets them so): a count
    // >= 2^31 reads as negative, wraps past the span and runs nothing.  (Why this order and this form: DESIGN.md 5.)
    const int cnt = T.n_dev ? (int)*T.n_dev : T.n;
    if ((unsigned)cnt - (unsigned)T.lo > (unsigned)T.hi - (unsigned)T.lo) return;  // not lo <= cnt <= hi; block-uniform, before any barrier
    T.n = cnt < T.n ? cnt : T.n;
    if (pos0 >= T.n) return;
    if (T.tally && blockIdx.x == 0 && tid == 0) atomicAdd(T.tally, 1u);
    [[maybe_unused]] unsigned long long tacc[4] = {0, 0, 0, 0}, tk0 = 0, tk1 = 0, tr0 = 0, tr1 = 0;
    BZ_STAMP(tk0);
#ifdef BZ_EXP_STAMPS
    tr0 = __builtin_amdgcn_s_memrealtime();
#endif
    char* bufX = smem;
    char* bufM = smem + G::BUF;
    const int r = lane & 31, h = lane >> 5;

    // ---- zero cells (conv halo: cell indices 0, 9, .., 72 of every position) of both buffers
    constexpr int ZC = G::CELL / 16;  // 16-byte chunks per cell
    for (int i = tid; i < 2 * P * 9 * ZC; i += 256) {
        int k = i % ZC, j = (i / ZC) % 9, pb = i / (9 * ZC);  // pb = buffer * P + position: BUF = P * TILE
        *reinterpret_cast<uint4*>(smem + pb * G::TILE + j * G::ROWC * G::CELL + k * 16) = make_uint4(0, 0, 0, 0);
    }
    // weight-fragment stream of this wave: k-step ks, M-tile mt -> wf[(ks * MT + mt) * 64 + lane], linear over layers
    const int wt0 = G::wt0(w), wp0 = G::pos0(w);
    // wave-uniform base (scalar registers) + lane: the loads take the SGPR-base addressing mode, so advancing the stream
    // costs scalar adds instead of 64-bit vector adds between the MFMAs
    const uint4* ap = G::M16 ? T.wf16 + (size_t)wt0 * 2 * 64 : T.wf + (size_t)wt0 * 64;
    typename WSetsOf<G>::type WS;
    if constexpr (G::M16) {  // tap 0 of the first layer: KQ steps x 2 channel halves
#pragma unroll
        for (int kq = 0; kq < G::KQ; ++kq)
#pragma unroll
            for (int a = 0; a < 2; ++a) WS.s[0][kq][a] = __builtin_bit_cast(bf16x8, ap[(kq * G::MT * 2 + a) * 64 + (unsigned)lane]);
        ap += G::KQ * G::MT * 2 * 64;
    } else {
#pragma unroll
        for (int d = 0; d + 1 < G::DEPTH; ++d) {  // chunks 0 .. DEPTH - 2 of the first layer
#pragma unroll
            for (int kc = 0; kc < G::KS; ++kc)
#pragma unroll
                for (int mt = 0; mt < MW; ++mt) WS.s[d][kc][mt] = __builtin_bit_cast(bf16x8, ap[(kc * G::MT + mt) * 64 + (unsigned)lane]);
            ap += G::KS * G::MT * 64;
        }
    }

    // ---- stem: conv3x3 2 -> C as a [C x 32] x [32 x 64] GEMM per position
    if constexpr (G::EDGE) {  // as the 16x16x32 stem below, one MFMA pair per tile of bz_tile_map.h: lane column c feeds pair c
        namespace tmap = bz_tile_map;
        f32x16 acc[MW][G::NU];
        Bias<G> bias;
        const int c = lane & 15, g = lane >> 4;
        load_bias16<G>(bias, T.stem_b, wt0, g);
        bf16x8 sa[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) sa[a] = __builtin_bit_cast(bf16x8, T.stem_wf16[(wt0 * 2 + a) * 64 + lane]);
        // the boards of the lane's positions: the row pattern serves two position pairs, the other patterns one position each
        const int lp[5] = {tmap::lane_p(tmap::kRow, c), 2 + tmap::lane_p(tmap::kRow, c), tmap::lane_p(tmap::kCol, c),
                           tmap::lane_p(tmap::kMix, c), tmap::lane_p(tmap::kIn, c)};
        u64 own[5], opp[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            int pos = pos0 + wp0 + lp[i];
            pos = pos < T.n ? pos : T.n - 1;
            own[i] = T.own[pos]; opp[i] = T.opp[pos];
        }
#pragma unroll
        for (int u = 0; u < G::NU; ++u) {
            acc[0][u] = (f32x16)(0.0f);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int t = 2 * u + b, i = t < 4 ? (t & 1) : 1 + tmap::pattern(t);
                const int cell = 8 * tmap::pair_y(t, c) + tmap::pair_x(t, c);
                const bf16x8 f = stem_frag16(nbhd(own[i], cell), nbhd(opp[i], cell), g);
                if (b) { mfma16_quarter<1>(acc[0][u], sa[0], f); mfma16_quarter<3>(acc[0][u], sa[1], f); }
                else { mfma16_quarter<0>(acc[0][u], sa[0], f); mfma16_quarter<2>(acc[0][u], sa[1], f); }
            }
        }
        epilogue_edge<G>(acc, bufX + wp0 * G::TILE, false, bias, wt0, lane);
    } else if constexpr (G::M16) {  // K = 32 is ONE 16x16x32 MFMA per quarter: lane (c, g) feeds cell c of half b with k = 8g ..
        f32x16 acc[MW][G::NU];
        Bias<G> bias;
        const int c = lane & 15, g = lane >> 4;
        load_bias16<G>(bias, T.stem_b, wt0, g);
        bf16x8 sa[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) sa[a] = __builtin_bit_cast(bf16x8, T.stem_wf16[(wt0 * 2 + a) * 64 + lane]);
        u64 own[2], opp[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            int pos = pos0 + wp0 + 2 * b + (c >> 3);
            pos = pos < T.n ? pos : T.n - 1;
            own[b] = T.own[pos]; opp[b] = T.opp[pos];
#if BZ_NET_SYM
            {  // the lanes that feed one position load the same words, so they agree on s
                const u32 s = bz_sym::of(Y, own[b], opp[b]);
                own[b] = bz_sym::board(own[b], Y.size, s); opp[b] = bz_sym::board(opp[b], Y.size, s);
            }
#endif
        }
#pragma unroll
        for (int u = 0; u < G::NU; ++u) {
            acc[0][u] = (f32x16)(0.0f);
            const int cell = 8 * u + (c & 7);
            const bf16x8 f0 = stem_frag16(nbhd(own[0], cell), nbhd(opp[0], cell), g);
            const bf16x8 f1 = stem_frag16(nbhd(own[1], cell), nbhd(opp[1], cell), g);
            mfma16_quarter<0>(acc[0][u], sa[0], f0);
            mfma16_quarter<1>(acc[0][u], sa[0], f1);
            mfma16_quarter<2>(acc[0][u], sa[1], f0);
            mfma16_quarter<3>(acc[0][u], sa[1], f1);
        }
        epilogue16<G>(acc, bufX + wp0 * G::TILE, false, bias, wt0, lane);
    } else {
        f32x16 acc[MW][G::NU];
        Bias<G> bias;
        load_bias<G>(bias, T.stem_b, wt0, h);
        bf16x8 sa[2][MW];
#pragma unroll
        for (int kc = 0; kc < 2; ++kc)
#pragma unroll
            for (int mt = 0; mt < MW; ++mt) sa[kc][mt] = __builtin_bit_cast(bf16x8, T.stem_wf[(kc * G::MT + wt0 + mt) * 64 + lane]);
        constexpr int NB = G::ROWT ? 1 : PW;  // row-tile units: every lane feeds ONE position (r >> 3) in all units
        u64 own[NB], opp[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            int pos = pos0 + wp0 + (G::ROWT ? r >> 3 : i);
            pos = pos < T.n ? pos : T.n - 1;
            own[i] = T.own[pos]; opp[i] = T.opp[pos];
#if BZ_NET_SYM
            {
                const u32 s = bz_sym::of(Y, own[i], opp[i]);
                own[i] = bz_sym::board(own[i], Y.size, s); opp[i] = bz_sym::board(opp[i], Y.size, s);
            }
#endif
        }
#pragma unroll
        for (int u = 0; u < G::NU; ++u) {
            const int i = G::ROWT ? 0 : u >> 1;
            const int cell = G::unit_cell(u, r);
            const unsigned n_own = nbhd(own[i], cell), n_opp = nbhd(opp[i], cell);
            bf16x8 sf[2] = {stem_frag<0>(n_own, n_opp, h), stem_frag<1>(n_own, n_opp, h)};
#pragma unroll
            for (int mt = 0; mt < MW; ++mt) {
                acc[mt][u] = (f32x16)(0.0f);
#pragma unroll
                for (int kc = 0; kc < 2; ++kc)
                    acc[mt][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sa[kc][mt], sf[kc], acc[mt][u], 0, 0, 0);
            }
        }
        epilogue<G>(acc, bufX + wp0 * G::TILE, false, bias, wt0, r, h);
    }
    __syncthreads();

    // ---- tower: a residual block = conv1 (X -> M) + conv2 (M -> X in place, + skip X)
#pragma unroll 1
    for (int blk = 0; blk < T.n_layers / 2; ++blk) {
        conv_layer<0, G>(bufX, bufM, false, T.bias + (size_t)(2 * blk) * C, WS, ap, w, r, h, tacc);
        conv_layer<G::NCH % G::DEPTH, G>(bufM, bufX, true, T.bias + (size_t)(2 * blk + 1) * C, WS, ap, w, r, h, tacc);
    }
    BZ_STAMP(tk1);

    // ---- heads: wave w serves positions w, w + 4, ...  conv1x1 (policy 2 ch + value 1 ch) by MFMA against
    // the resident tile, then the FCs in fp32 with the position's 192 features staged in LDS (M is dead now).
    float* S = reinterpret_cast<float*>(bufM + w * 1024);  // [pf 128 | vf 64], one scratch per wave
    const float pb0 = T.pol_b[0], pb1 = T.pol_b[1], vb = T.val_b[0];
    bf16x8 hw[G::KC];  // all head-conv fragments in flight at once (one L2 round trip, not one per MFMA)
#pragma unroll
    for (int kc = 0; kc < G::KC; ++kc) hw[kc] = __builtin_bit_cast(bf16x8, T.head_wf[kc * 64 + lane]);
    for (int p = w; p < P && pos0 + p < T.n; p += 4) {
        const int pos = pos0 + p;
#if BZ_NET_SYM  // the head wave recomputes its position's s; logit a goes to the cell that T_s moved onto a
        const int dst = bz_sym::tau_inv(Y.size, bz_sym::of(Y, T.own[pos], T.opp[pos]), lane);
#else
        const int dst = lane;
#endif
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            f32x16 acc = (f32x16)(0.0f);
            const int cell = 32 * nt + r;
#pragma unroll
            for (int kc = 0; kc < G::KC; ++kc) {
                bf16x8 b = *reinterpret_cast<const bf16x8*>(bufX + p * G::TILE + G::cell_off(p, cell, 2 * kc + h));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hw[kc], b, acc, 0, 0, 0);
            }
            if (h == 0) {  // rows 0..2 of D live in registers 0..2 of lanes 0..31
                float a0 = acc[0] + pb0, a1 = acc[1] + pb1, a2 = acc[2] + vb;
                S[cell] = relu_f32(a0);
                S[64 + cell] = relu_f32(a1);
                S[128 + cell] = relu_f32(a2);
            }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's own LDS writes have landed
        // policy FC 128 -> 65: lane a owns logit a; logit 64 (pass) is a wave reduction
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
        // value FC 64 -> VH -> 1, tanh
        float vh = 0.0f;
        if (lane < T.VH) {
            float a = T.v1_b[lane];
#pragma unroll 32
            for (int i = 0; i < 64; ++i) a = __builtin_fmaf(S[128 + i], T.v1_wT[i * T.VH + lane], a);
            vh = relu_f32(a) * T.v2_w[lane];
        }
        vh = wave_sum(vh);
        if (lane == 0) T.value[pos] = tanhf_spec(vh + T.v2_b[0]);
        __builtin_amdgcn_s_waitcnt(0xC07F);  // the scratch is reused for the wave's next position
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
