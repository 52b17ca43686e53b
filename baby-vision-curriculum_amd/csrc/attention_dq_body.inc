// Body of attn_bwd_dq_kernel / attn_bwd_dq_win_kernel (attention.hip): see attention_fwd_body.inc.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int HI = img_hd(HD);
    constexpr int IMG = 64 * HI * 2, STG = 2 * IMG, SUB = 32 * HI * 2;
    const AS3 char* lds = (const AS3 char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NQ = WIN ? Nq_ : N, q_off = WIN ? q_off_ : 0;
    const int ztiles = WIN ? (q_off + 127) >> 7 : 0;
    int tile_, bh;
    attn_block(((NQ + 127) >> 7) + ztiles, remap, tile_, bh);
    const int b = bh / H, head = bh % H;
    const int ld = 3 * D;
    if constexpr (WIN) {
        if (tile_ < ztiles) {      // workgroup-uniform, before any barrier: two threads per row, HD bytes each
            const int r = tile_ * 128 + (tid >> 1);
            if (r < q_off) {
                uint2* z = reinterpret_cast<uint2*>(dqkv + (size_t)(b * N + r) * ld + head * HD + (tid & 1) * (HD / 2));
#pragma unroll
                for (int i = 0; i < HD / 8; ++i) z[i] = uint2{0u, 0u};
            }
            return;
        }
        tile_ -= ztiles;
    }
    const TailSplit ts = tail_split(NQ, tile_, wave);      // the ragged last block: idle waves share the key loop of the owners
    const int qi = tile_ * 128 + ts.own * 32 + (lane & 31);
    const int qc = min(qi, NQ - 1);
    const int h = lane >> 5;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(qkv, qkv_bytes);
    const FragAddr<HI> fa = make_frag_addr<HI>(lane);
    const int gm = ts.gs - 1;
    auto mine = [&](int sub) { return (sub & gm) == ts.part; };

    bf16x8 qf[HI / 16], dof[HI / 16];
    float del_q = 0.f;
    {
        const bf16_t* qrow = qkv + (size_t)(b * N + q_off + qc) * ld + head * HD + 8 * h;
        const bf16_t* drow = dctx + (size_t)(b * NQ + qc) * D + head * HD + 8 * h;
        const bf16_t* orow_in = ctx + (size_t)(b * NQ + qc) * D + head * HD + 8 * h;
#pragma unroll
        for (int st = 0; st < HI / 16; ++st) {
            qf[st] = load8_head<HD, HI>(qrow + 16 * st, 16 * st + 8 * h);
            dof[st] = load8_head<HD, HI>(drow + 16 * st, 16 * st + 8 * h);
            // delta = rowsum(dO * O) of this query (the softmax-gradient correction): the two half-waves hold disjoint halves
            // of the row, so it costs one more 16-B load per step here instead of a pass of its own over dO and O
            const bf16x8 of = load8_head<HD, HI>(orow_in + 16 * st, 16 * st + 8 * h);     // (past the head: 0 * 0 terms)
#pragma unroll
            for (int j = 0; j < 8; ++j) del_q += bf2f((bf16_t)dof[st][j]) * bf2f((bf16_t)of[j]);
        }
    }
    del_q += __shfl_xor(del_q, 32, 64);
    if (h == 0 && qi < NQ && ts.part == 0) delta[(size_t)bh * NQ + qi] = -del_q;     // NEGATED: the dK/dV kernel, launched after this one, starts its dP chain from it
    float nlse = -lse[(size_t)bh * NQ + qc];
#pragma unroll
    for (int stq = 0; stq < HI / 16; ++stq) { settle(qf[stq]); settle(dof[stq]); }
    settle(nlse); settle(del_q);
    f32x16 ndel;
#pragma unroll
    for (int r = 0; r < 16; ++r) ndel[r] = -del_q;
    f32x16 dq[HI / 32];
#pragma unroll
    for (int t = 0; t < HI / 32; ++t) dq[t] = zero16();

    const int nkt = (N + 63) >> 6;
    const int krow0 = b * N;
    auto issue = [&](int kt, int stage) {
        stage64<HI, 4, HD>(rs, krow0 + kt * 64, ld, D + head * HD, smem + stage * STG, wave, lane);
        stage64<HI, 4, HD>(rs, krow0 + kt * 64, ld, 2 * D + head * HD, smem + stage * STG + IMG, wave, lane);
    };
    issue(0, 0);
    for (int kt = 0; kt < nkt; kt += 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nkt) issue(kt + 1, 1);
        if (mine(2 * kt)) dq_subtile<HI, 0, IMG>(lds, fa, qf, dof, dq, kt * 64, N, h, scale_log2, nlse, ndel);
        if (kt * 64 + 32 < N && mine(2 * kt + 1)) dq_subtile<HI, SUB, IMG + SUB>(lds, fa, qf, dof, dq, kt * 64 + 32, N, h, scale_log2, nlse, ndel);
        if (kt + 1 >= nkt) break;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 2 < nkt) issue(kt + 2, 0);
        if (mine(2 * kt + 2)) dq_subtile<HI, STG, STG + IMG>(lds, fa, qf, dof, dq, kt * 64 + 64, N, h, scale_log2, nlse, ndel);
        if (kt * 64 + 96 < N && mine(2 * kt + 3))
            dq_subtile<HI, STG + SUB, STG + IMG + SUB>(lds, fa, qf, dof, dq, kt * 64 + 96, N, h, scale_log2, nlse, ndel);
    }
    if (ts.gs > 1) tail_reduce<HI / 32>(smem, ts, lane, dq);
    if (qi < NQ && ts.part == 0) {
        bf16_t* orow = dqkv + (size_t)(b * N + q_off + qi) * ld + head * HD;
#pragma unroll
        for (int t = 0; t < HI / 32; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * t + 8 * g + 4 * h;
                if (HD != HI && d >= HD) continue;
                uint2 a = {pack2bf(dq[t][4 * g] * scale, dq[t][4 * g + 1] * scale), pack2bf(dq[t][4 * g + 2] * scale, dq[t][4 * g + 3] * scale)};
                *reinterpret_cast<uint2*>(orow + d) = a;
            }
    }
