// The two production channelisers, k_channelize and k_channelize_kur (k_channelize.hip), written once and
// included three times: CH_COH 0 = power planes -- CH_INJ 0 without any FRB injection code (the kernels named
// k_channelize, k_channelize_kur), CH_INJ 1 with it (k_inject_chan, k_inject_chan_kur: launched only when a pulse is
// to be injected) -- and CH_COH 1 = the complex spectra of coherence output (k_coh_chan, k_coh_chan_kur, CH_INJ 1).
// CH_K_PLAIN / CH_K_KUR name the kernels.
// The coherence twins keep the float2 of every channel until it is stored: within the 168 registers of three
// workgroups per CU that spilled, so they are built for two (256 registers; the LDS would hold three).
#define CH_WG_PER_CU (CH_COH ? 2 : 3)

#if defined(FFT_LEAN) && !CH_COH
// (dynamic LDS: with a static 50-KB buffer the compiler sees three workgroups per CU and takes 168 registers)
__global__ __launch_bounds__(256, 4) void CH_K_PLAIN(ChanArgs a)
{
    extern __shared__ __attribute__((aligned(16))) f2 buf[];
#else
__global__ __launch_bounds__(256, CH_WG_PER_CU) void CH_K_PLAIN(ChanArgs a)
{
    __shared__ __attribute__((aligned(16))) f2 buf[M_HALF];
#endif
    FFT_STAMP(8);
    int tid = threadIdx.x;
    // grid (ceil(R / CH_ROWS), nseg * 2, A): no division to find the rows
    const int row0 = blockIdx.x * CH_ROWS, seg = blockIdx.y >> 1, pol = blockIdx.y & 1, ant = blockIdx.z;
    const int nrow = min(CH_ROWS, a.R - row0);

    // The first row's bytes are requested first; the rows' flag masks and weights (written by the kurtosis kernel:
    // lane i of every wave fetches the mask of row i, lane CH_ROWS + i its weight) follow, so that neither latency
    // precedes the other (25 flag bytes fetched before any sample was requested cost 1.7 us per workgroup).
    RowStage st;
    stage_request(a, tid, seg, row0, pol, ant, st);
    unsigned vmw = 0;
    if (a.rfi_mode) {
        const int l = tid & 63, i = l % CH_ROWS;
        const size_t wi = (size_t)ant * a.wrow_ant_stride + (size_t)seg * a.R + row0 + i;
        if (l < 2 * CH_ROWS && i < nrow) vmw = l < CH_ROWS ? a.rowmask[wi] : __builtin_bit_cast(unsigned, a.wrow[wi]);
    }
#pragma unroll 1
    for (int i = 0; i < nrow; ++i) {
        const int row = row0 + i;
        const int after = i + 1 < nrow ? row + 1 : -1;
        // row weight exactly as apply_kurtosis accumulates it: one 500/12500 per unflagged block
        const unsigned mask = __builtin_amdgcn_readlane(vmw, i);
        const float wrow = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vmw, CH_ROWS + i));
        const size_t prow = (size_t)ant * a.p_ant_stride + (((size_t)seg * 2 + pol) * a.R + row) * PB_NCHANOUT;
        const bool all_bad = mask == 0x1ffffffu;
        // transforms of this row: role 0 = raw spectrum (an unflagged row's excised power is derived from it
        // downstream), role 1 = excised spectrum (only when some block is flagged: 13 % of rows on clean
        // noise), instead of launching a second grid of workgroups of which 87 % would exit at once.
        const bool second = a.rfi_mode == 1 || (a.rfi_mode == 2 && mask != 0);
        if (i) __syncthreads();   // the previous transform has finished reading buf
        if (a.rfi_mode != 1) {
            channelize_pass<0, false, false, CH_COH, CH_INJ>(a, buf, tid, seg, row, pol, ant, st, mask, wrow, prow,
                                                     second && !all_bad ? row : after);
            if (!second) continue;
        }
        if (all_bad) {
            // weight 0: the row's excised power is never used for its value (detect_and_normalize3
            // :474-476 writes 0 and leaves the bandpass alone); +inf makes the detect kernel's clip test
            // do exactly that without having to look at the weight
            if constexpr (CH_COH)
                for (int c = tid; c < PB_NCHANOUT; c += 256) ((float2 *)a.Pkur)[prow + c] = make_float2(0.f, 0.f);
            else
                for (int c = tid; c < PB_NCHANOUT; c += 256) a.Pkur[prow + c] = __builtin_inff();
            if (a.rfi_mode == 1 && after >= 0) stage_request(a, tid, seg, after, pol, ant, st);
            continue;
        }
        if (a.rfi_mode == 2) {
            __syncthreads();   // the raw pass has finished reading buf
            asm volatile("" : "+v"(tid));   // no sharing of tid-derived addresses across the two passes
        }
        channelize_pass<1, false, false, CH_COH, CH_INJ>(a, buf, tid, seg, row, pol, ant, st, mask, wrow, prow, after);
    }
}


__global__ __launch_bounds__(256, CH_WG_PER_CU) void CH_K_KUR(ChanArgs a)
{
    __shared__ __attribute__((aligned(16))) f2 buf[M_HALF];
    __shared__ unsigned smw[2];     // the row's flag mask and weight bits (outside buf: the transforms overwrite that)
#ifdef KUR_STAMP
    __shared__ unsigned long long kts[8];
#endif
    KSTAMP(0);
#ifdef KUR_STAMP
    if (threadIdx.x == 0) kts[6] = __builtin_amdgcn_s_memrealtime();
#endif
    int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = blockIdx.x, seg = blockIdx.y, ant = blockIdx.z;
    const int grow = seg * a.R + row;

    // both rows' bytes go to LDS, patched for code 0, for the statistics; pol 0's stay where its first transform
    // expects them (the start of buf), so that transform stages nothing
    RowStage st;
    unsigned off0, off1;
    DagConsts dc;
    uint4 *sraw0 = (uint4 *)buf, *sraw1 = (uint4 *)buf + 784;     // 2 x 12 544 B
    float *s2 = (float *)((uint4 *)buf + 2 * 784), *s4 = s2 + 50;
    {
        RowStage sb;
        stage_request(a, tid, seg, row, 0, ant, st);
        stage_request(a, tid, seg, row, 1, ant, sb);
#ifndef KUR_NO_DAG_PREFETCH
        // the D'Agostino constants are requested with the rows: their first use is on the critical path of the wave
        // that decides the flags, and a scalar load from memory is a microsecond there
        dc = *a.dag;
#endif
        off0 = (unsigned)(row_byte(a, seg, row, 0, ant) & 15);
        off1 = (unsigned)(row_byte(a, seg, row, 1, ant) & 15);
        const bool l0 = tid + 768 < (int)((off0 + PB_NFFT + 15) >> 4), l1 = tid + 768 < (int)((off1 + PB_NFFT + 15) >> 4);
        sraw0[tid] = fix_zero_codes(st.t0);
        sraw0[tid + 256] = fix_zero_codes(st.t1);
        sraw0[tid + 512] = fix_zero_codes(st.t2);
        if (l0) sraw0[tid + 768] = fix_zero_codes(st.t3);
        sraw1[tid] = fix_zero_codes(sb.t0);
        sraw1[tid + 256] = fix_zero_codes(sb.t1);
        sraw1[tid + 512] = fix_zero_codes(sb.t2);
        if (l1) sraw1[tid + 768] = fix_zero_codes(sb.t3);
    }
    __syncthreads();
    KSTAMP(1);
    // moments of the 50 blocks: k_kurtosis_row's reduction (kurtosis_dev.h)
    row_block_moments((const uint8_t *)sraw0 + off0, (const uint8_t *)sraw1 + off1, wave, lane, s2, s4);
    __syncthreads();
    KSTAMP(2);
    // The flags are the business of ONE wave: lanes 0..49 decide their block's flag (no cube root, kurtosis_dev.h), a
    // ballot brings the two pols together (bit b of the mask = block b flagged in pol 0 or pol 1: compute_dagostino's
    // max over pols, :109-134), lane 0 books the weight.  The other waves go straight on to unpacking pol 0, whose
    // bytes are where the transform expects them; the mask and the weight are first needed after that transform's FFT
    // (RFI mode 2), and they reach the other waves through `smw` across the barrier that precedes pass 1 -- which
    // also keeps pass 1 from overwriting the moments before this wave has read them.
    if (wave == 0) {
        bool f = false;
        if (lane < 50) {
            const float p = s2[lane] / PB_NKURTO;
            const float k = s4[lane] / PB_NKURTO / (p * p);
#ifndef KUR_NO_DAG_PREFETCH
            f = dag_flag(k, dc);
#else
            f = dag_flag(k, *a.dag);
#endif
        }
        const unsigned long long b = __ballot(f);
        const uint32_t m = (uint32_t)((b | (b >> 25)) & 0x1ffffffull);
        if (lane < 25) a.flags[(size_t)ant * a.flags_ant_stride + (size_t)grow * PB_BLK_PER_FFT + lane] = (m >> lane) & 1u;
        if (lane == 0) {
            // kur_weights after apply_kurtosis (:292): one 500/12500 per unflagged block, summed left to right
            const float inc = (float)PB_NKURTO / PB_NFFT;
            float w = 0.f;
            for (int k = PB_BLK_PER_FFT - __popc(m); k > 0; --k) w = w + inc;
            a.wrow_out[(size_t)ant * a.wrow_ant_stride + grow] = w;
            a.rowmask_out[(size_t)ant * a.wrow_ant_stride + grow] = m;
            smw[0] = m;
            smw[1] = __builtin_bit_cast(unsigned, w);
        }
    }
    KSTAMP(3);
    unsigned mask = 0;
    float wrow = 0.f;
    if (a.rfi_mode == 1) {
        // the excised transform zeroes flagged blocks while it unpacks: it needs the mask first
        __syncthreads();
        mask = __builtin_amdgcn_readfirstlane(smw[0]);
        wrow = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(smw[1]));
    }
    KSTAMP(4);

#pragma unroll 1
    for (int pol = 0; pol < 2; ++pol) {
        const size_t prow = (size_t)ant * a.p_ant_stride + (((size_t)seg * 2 + pol) * a.R + row) * PB_NCHANOUT;
        const int after_row = pol == 0 ? row : -1;         // what follows this pol's transforms: pol 1 of the same row
        if (pol) __syncthreads();   // the previous transform has finished reading buf
        if (a.rfi_mode != 1) {
            // what is requested while this transform is in its spectrum step -- the same row again for its excised
            // transform, else pol 1's row -- is decided inside, once the mask is known
            channelize_pass<0, true, true, CH_COH, CH_INJ>(a, buf, tid, seg, row, pol, ant, st, 0u, 0.f, prow, -1, 1, pol == 0, smw, after_row);
            mask = __builtin_amdgcn_readfirstlane(smw[0]);
            wrow = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(smw[1]));
        }
        const bool all_bad = mask == 0x1ffffffu;
        const bool second = a.rfi_mode == 1 || (a.rfi_mode == 2 && mask != 0);
        if (!second) continue;
        if (all_bad) {
            if constexpr (CH_COH)
                for (int c = tid; c < PB_NCHANOUT; c += 256) ((float2 *)a.Pkur)[prow + c] = make_float2(0.f, 0.f);
            else
                for (int c = tid; c < PB_NCHANOUT; c += 256) a.Pkur[prow + c] = __builtin_inff();
            if (a.rfi_mode == 1 && after_row >= 0) stage_request(a, tid, seg, after_row, 1, ant, st);
            continue;
        }
        if (a.rfi_mode == 2) {
            __syncthreads();   // the raw pass has finished reading buf
            asm volatile("" : "+v"(tid));   // no sharing of tid-derived addresses across the two passes
        }
        // (RFI mode 1, pol 0: the bytes the statistic staged are still where this transform expects them)
        channelize_pass<1, true, false, CH_COH, CH_INJ>(a, buf, tid, seg, row, pol, ant, st, mask, wrow, prow, after_row, 1,
                                 a.rfi_mode == 1 && pol == 0);
    }
#ifdef KUR_STAMP
    if (threadIdx.x == 0 && blockIdx.z == 0) {
        const unsigned wg = blockIdx.x + gridDim.x * blockIdx.y;
        if (wg < 10240) {
            unsigned long long(*g)[10] = g_kur_stamp[a.frb.since & 3];
            for (int i = 0; i < 5; ++i) g[wg][i] = kts[i];
            g[wg][5] = __builtin_amdgcn_s_memtime();
            g[wg][6] = mask;
            g[wg][7] = (unsigned long long)__builtin_amdgcn_s_getreg(20 | (3 << 11)) |       // HW_REG_XCC_ID
                       ((unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) << 8);  // HW_REG_HW_ID
            g[wg][8] = kts[6];
            g[wg][9] = __builtin_amdgcn_s_memrealtime();
        }
    }
#endif
}
#undef CH_WG_PER_CU
