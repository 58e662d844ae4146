// bz_train_fwd_body.h -- the training tower's forward kernel.  Included twice by bz_train.hip, inside its anonymous namespace:
// with BZ_TRAIN_QAT 0 it defines k_train_fwd<G>, with BZ_TRAIN_QAT 1 k_qat_fwd, the fp8 net's forward for quantisation-aware
// training: the 128-channel geometry with the activation rule of bz_qat.h in every layer's epilogue; act[0]
// comes from k_qat_stem and the weight stream from k_qat_pack, so every operand of the bf16 MFMAs is a value of the fp8 net,
// exactly.  One text, two kernels -- not a shared inlined body (bz_net_tower_fp8_body.h): k_train_fwd then compiles to the very
// instructions it had before, and the resource tests find one kernel per name.
#if BZ_TRAIN_QAT
__global__ void __launch_bounds__(256, 1) k_qat_fwd(TrainArgs T) {
    typedef Tw<128, 4, true> G;
#else
template <class G>
__global__ void __launch_bounds__(256, 1) k_train_fwd(TrainArgs T) {
#endif
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pos0 = blockIdx.x * G::P, r = lane & 31, h = lane >> 5;
    if (pos0 >= T.n) return;
    [[maybe_unused]] unsigned long long tacc[4] = {0, 0, 0, 0};
    char* bufX = smem;
    char* bufM = smem + G::BUF;
    zero_halo<G>(smem, tid);
    const uint4* ap = T.wf + (size_t)G::wt0(w) * (G::M16 ? 2 * 64 : 64);
    typename WSetsOf<G>::type WS;
    weights_prologue<G>(WS, ap, lane);
    load_tile<G>(bufX, T.in, pos0, tid);
    __syncthreads();
    const size_t slot = (size_t)T.n * 64 * G::C;                       // elements of one activation tensor
    __bf16* const mine = T.out + (size_t)pos0 * 64 * G::C;             // the workgroup's positions in the first output tensor
    const size_t mslot = (size_t)(T.n / G::P) * 256;                    // mask words of one layer
    uint4* mk = T.masks + (size_t)blockIdx.x * 256 + tid;
#pragma unroll 1
    for (int blk = 0; blk < T.n_layers / 2; ++blk) {
        unsigned bits[4];
        // (act[2 blk] = X, the previous block's result, leaves in this layer's epilogue; act[0] came from HBM)
        conv_layer<0, G>(bufX, bufM, false, T.bias + (size_t)(2 * blk) * G::C, WS, ap, w, r, h, tacc,
                         EpTrain<G, false, BZ_TRAIN_QAT != 0>{bits, true, bufX, blk > 0 ? mine + (size_t)(2 * blk - 1) * slot : nullptr, tid});
        if constexpr (!kCopyInEpilogue<G>)
            if (__bf16* cd = blk > 0 ? mine + (size_t)(2 * blk - 1) * slot : nullptr) store_tile<G>(bufX, cd, 0, tid);
        mk[(size_t)(2 * blk) * mslot] = make_uint4(bits[0], bits[1], bits[2], bits[3]);
        conv_layer<G::NCH % G::DEPTH, G>(bufM, bufX, true, T.bias + (size_t)(2 * blk + 1) * G::C, WS, ap, w, r, h, tacc,
                                         EpTrain<G, false, BZ_TRAIN_QAT != 0>{bits, true, bufM, mine + (size_t)(2 * blk) * slot, tid});
        if constexpr (!kCopyInEpilogue<G>)
            if (__bf16* cd = mine + (size_t)(2 * blk) * slot) store_tile<G>(bufM, cd, 0, tid);
        mk[(size_t)(2 * blk + 1) * mslot] = make_uint4(bits[0], bits[1], bits[2], bits[3]);
    }
    store_tile<G>(bufX, mine + (size_t)(T.n_layers - 1) * slot, 0, tid);
}
