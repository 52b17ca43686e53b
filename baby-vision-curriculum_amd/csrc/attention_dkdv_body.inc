// Body of attn_bwd_dkdv_kernel / attn_bwd_dkdv_win_kernel (attention.hip): see attention_fwd_body.inc.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int NQ = WIN ? Nq_ : N, q_off = WIN ? q_off_ : 0;
    constexpr int HI = img_hd(HD);
    constexpr int IMG = 64 * HI * 2, SUB = 32 * HI * 2, STG = 2 * IMG + 512;
    const AS3 char* lds = (const AS3 char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int tile_, bh;
    attn_block((N + 127) >> 7, remap, tile_, bh);
    const int b = bh / H, head = bh % H;
    const int ld = 3 * D;
    const TailSplit ts = tail_split(N, tile_, wave);      // the ragged last key block: idle waves share the query loop of the owners
    const int ki = tile_ * 128 + ts.own * 32 + (lane & 31);   // this lane's key
    const int kc = min(ki, N - 1);
    const int h = lane >> 5;
    const int gm = ts.gs - 1;
    auto mine = [&](int sub) { return (sub & gm) == ts.part; };
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(qkv, qkv_bytes);
    const __amdgpu_buffer_rsrc_t rd = make_rsrc(dctx, dctx_bytes);
    const __amdgpu_buffer_rsrc_t rl = make_rsrc(lse, stat_bytes);
    const __amdgpu_buffer_rsrc_t re = make_rsrc(delta, stat_bytes);
    const FragAddr<HI> fa = make_frag_addr<HI>(lane);

    bf16x8 kf[HI / 16], vf[HI / 16];   // B operands of S = Q K^T and dP = dO V^T
    {
        const bf16_t* krow = qkv + (size_t)(b * N + kc) * ld + D + head * HD + 8 * h;
#pragma unroll
        for (int st = 0; st < HI / 16; ++st) {
            kf[st] = load8_head<HD, HI>(krow + 16 * st, 16 * st + 8 * h);
            vf[st] = load8_head<HD, HI>(krow + D + 16 * st, 16 * st + 8 * h);
        }
    }
#pragma unroll
    for (int stq = 0; stq < HI / 16; ++stq) { settle(kf[stq]); settle(vf[stq]); }
    f32x16 dk[HI / 32], dv[HI / 32];
#pragma unroll
    for (int t = 0; t < HI / 32; ++t) { dk[t] = zero16(); dv[t] = zero16(); }

    const int nqt = (NQ + 63) >> 6;
    const int qrow0 = b * N + q_off, drow0 = b * NQ;
    auto issue = [&](int qt, int stage) {
        char* dst = smem + stage * STG;
        stage64<HI, 4, HD>(rq, qrow0 + qt * 64, ld, head * HD, dst, wave, lane);
        stage64<HI, 4, HD>(rd, drow0 + qt * 64, D, head * HD, dst + IMG, wave, lane);
        if (wave == 0)
            glds4(rl, (uint32_t)(((size_t)bh * NQ + qt * 64 + lane) * 4), (uint32_t)(size_t)((AS3 char*)dst) + 2 * IMG);
        if (wave == 1)
            glds4(re, (uint32_t)(((size_t)bh * NQ + qt * 64 + lane) * 4), (uint32_t)(size_t)((AS3 char*)dst) + 2 * IMG + 256);
    };
    issue(0, 0);
    for (int qt = 0; qt < nqt; qt += 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (qt + 1 < nqt) issue(qt + 1, 1);
        if (mine(2 * qt)) dkdv_subtile<HI, 0, 2 * IMG>(lds, fa, kf, vf, dk, dv, qt * 64, NQ, h, scale_log2);
        if (qt * 64 + 32 < NQ && mine(2 * qt + 1)) dkdv_subtile<HI, SUB, 2 * IMG + 128>(lds, fa, kf, vf, dk, dv, qt * 64 + 32, NQ, h, scale_log2);
        if (qt + 1 >= nqt) break;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (qt + 2 < nqt) issue(qt + 2, 0);
        if (mine(2 * qt + 2)) dkdv_subtile<HI, STG, STG + 2 * IMG>(lds, fa, kf, vf, dk, dv, qt * 64 + 64, NQ, h, scale_log2);
        if (qt * 64 + 96 < NQ && mine(2 * qt + 3)) dkdv_subtile<HI, STG + SUB, STG + 2 * IMG + 128>(lds, fa, kf, vf, dk, dv, qt * 64 + 96, NQ, h, scale_log2);
    }
    if (ts.gs > 1) {      // (one accumulator set at a time: three partial sets of 8 KiB fit the 33 KiB ring, six do not)
        tail_reduce<HI / 32>(smem, ts, lane, dk);
        tail_reduce<HI / 32>(smem, ts, lane, dv);
    }
    if (ki < N && ts.part == 0) {
        bf16_t* krow = dqkv + (size_t)(b * N + ki) * ld + D + head * HD;
        bf16_t* vrow = krow + D;
#pragma unroll
        for (int t = 0; t < HI / 32; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * t + 8 * g + 4 * h;
                if (HD != HI && d >= HD) continue;
                uint2 a = {pack2bf(dk[t][4 * g] * scale, dk[t][4 * g + 1] * scale), pack2bf(dk[t][4 * g + 2] * scale, dk[t][4 * g + 3] * scale)};
                *reinterpret_cast<uint2*>(krow + d) = a;
                uint2 e = {pack2bf(dv[t][4 * g], dv[t][4 * g + 1]), pack2bf(dv[t][4 * g + 2], dv[t][4 * g + 3])};
                *reinterpret_cast<uint2*>(vrow + d) = e;
            }
    }
