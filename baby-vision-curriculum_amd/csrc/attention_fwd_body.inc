// Body of attn_fwd_kernel / attn_fwd_win_kernel (attention.hip), included into both so that each is compiled as a kernel of its own:
// expects the kernel arguments, `constexpr bool WIN` and, for the window, `q_off_` / `Nq_` in scope.
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 stages x (K image + V image)
    const int NQ = WIN ? Nq_ : N, q_off = WIN ? q_off_ : 0;
    constexpr int HI = img_hd(HD);   // the image width (96 for 80 / 88)
    constexpr int IMG = 64 * HI * 2, STG = 2 * IMG, SUB = 32 * HI * 2;
    const AS3 char* lds = (const AS3 char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int tile_, bh;
    attn_block((NQ + 32 * NW - 1) / (32 * NW), remap, tile_, bh);
    const int b = bh / H, head = bh % H;
    const int ld = 3 * D;
    const TailSplit ts = tail_split<NW>(NQ, tile_, wave);
    const int qi = tile_ * (32 * NW) + ts.own * 32 + (lane & 31);   // this lane's query (inside the window)
    const int h = lane >> 5;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(qkv, qkv_bytes);
    const FragAddr<HI> fa = make_frag_addr<HI>(lane);
    const int gm = ts.gs - 1;
    auto mine = [&](int sub) { return (sub & gm) == ts.part; };      // does this wave take 32-key sub-tile `sub`?

    bf16x8 qf[HI / 16];   // Q^T fragments (B operand of S^T = K Q^T): Q[qi][16 step + 8 h + 0..7]
    {
        const bf16_t* qrow = qkv + (size_t)(b * N + q_off + min(qi, NQ - 1)) * ld + head * HD + 8 * h;
#pragma unroll
        for (int st = 0; st < HI / 16; ++st) qf[st] = load8_head<HD, HI>(qrow + 16 * st, 16 * st + 8 * h);
    }
    FwdState<HI> st;
#pragma unroll
    for (int t = 0; t < HI / 32; ++t) st.o[t] = zero16();
    st.m_run = -INFINITY; st.l_run = 0.f;

    const int nkt = (N + 63) >> 6;
    const int krow0 = b * N;
    auto issue = [&](int kt, int stage) {
        stage64<HI, NW, HD>(rs, krow0 + kt * 64, ld, D + head * HD, smem + stage * STG, wave, lane);
        stage64<HI, NW, HD>(rs, krow0 + kt * 64, ld, 2 * D + head * HD, smem + stage * STG + IMG, wave, lane);
    };
#pragma unroll
    for (int stq = 0; stq < HI / 16; ++stq) settle(qf[stq]);
    issue(0, 0);
    for (int kt = 0; kt < nkt; kt += 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nkt) issue(kt + 1, 1);
        if (mine(2 * kt)) fwd_subtile<HI, 0, IMG>(lds, fa, qf, st, kt * 64, N, h, scale_log2);
        if (kt * 64 + 32 < N && mine(2 * kt + 1)) fwd_subtile<HI, SUB, IMG + SUB>(lds, fa, qf, st, kt * 64 + 32, N, h, scale_log2);
        if (kt + 1 >= nkt) break;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 2 < nkt) issue(kt + 2, 0);
        if (mine(2 * kt + 2)) fwd_subtile<HI, STG, STG + IMG>(lds, fa, qf, st, kt * 64 + 64, N, h, scale_log2);
        if (kt * 64 + 96 < N && mine(2 * kt + 3)) fwd_subtile<HI, STG + SUB, STG + IMG + SUB>(lds, fa, qf, st, kt * 64 + 96, N, h, scale_log2);
    }
    if (ts.gs > 1) {      // workgroup-uniform: merge the parts of a query tile (flash-decoding style: common maximum, rescaled sums)
        AS3 float* cl = (AS3 float*)smem;
        constexpr int NO = HI / 32 * 16, SLOT = (NO + 2) * 64;
        __syncthreads();
        if (ts.part > 0) {
            AS3 float* w = cl + ((ts.part - 1) * ts.valid + ts.own) * SLOT + lane;
#pragma unroll
            for (int t = 0; t < HI / 32; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) w[(t * 16 + r) * 64] = st.o[t][r];
            w[NO * 64] = st.m_run;
            w[(NO + 1) * 64] = st.l_run;
        }
        __syncthreads();
        if (ts.part == 0) {
            for (int p = 1; p < ts.gs; ++p) {
                const AS3 float* w = cl + ((p - 1) * ts.valid + ts.own) * SLOT + lane;
                const float m_p = w[NO * 64], l_p = w[(NO + 1) * 64];
                const float m_new = fmaxf(st.m_run, m_p);
                const float a = st.m_run == -INFINITY ? 0.f : fast_exp2(st.m_run - m_new);     // (a part that saw no key: -inf, weight 0)
                const float c = m_p == -INFINITY ? 0.f : fast_exp2(m_p - m_new);
                st.m_run = m_new;
                st.l_run = st.l_run * a + l_p * c;
#pragma unroll
                for (int t = 0; t < HI / 32; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) st.o[t][r] = st.o[t][r] * a + w[(t * 16 + r) * 64] * c;
            }
        }
    }
    const float l_tot = xhalf_sum(st.l_run);
    const float inv = 1.f / l_tot;
    if (qi < NQ && ts.part == 0) {
        bf16_t* orow = ctx + (size_t)(b * NQ + qi) * D + head * HD;
#pragma unroll
        for (int t = 0; t < HI / 32; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * t + 8 * g + 4 * h;
                if (HD != HI && d >= HD) continue;     // past a narrower head
                uint2 a = {pack2bf(st.o[t][4 * g] * inv, st.o[t][4 * g + 1] * inv), pack2bf(st.o[t][4 * g + 2] * inv, st.o[t][4 * g + 3] * inv)};
                *reinterpret_cast<uint2*>(orow + d) = a;
            }
        if (h == 0) lse[(size_t)bh * NQ + qi] = st.m_run + log2f(l_tot);
    }
