// background_sites_body.inc -- the body of the background site kernels (background.hip), included once per kernel:
// k_background_sites defines BG_RUN_BASE and BG_PRIMER_BASE empty (the whole stream, all primers), k_background_slab
// as "run_base +" and "primer_base +" (a slab of runs against a range of primers).  The text is the same for both, so
// the whole-stream kernels compile to what they were before the slab kernel existed.
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ uint32_t s_lo[kRunWords], s_hi[kRunWords], s_ok[kRunWords];
    T *tile = reinterpret_cast<T *>(smem);
    uint32_t *scnt = reinterpret_cast<uint32_t *>(smem + (size_t)tile_cap * sizeof(T));   // [2 i + s]
    const int tid = threadIdx.x;
    const size_t bw = (total_len + 31) / 32, vw2 = 2 * ((total_len + 63) / 64);
    const uint32_t *ok32 = reinterpret_cast<const uint32_t *>(packed + bw);   // validity, 32 columns per word
    const uint32_t kmask = (uint32_t)((1ull << k) - 1ull);
    const uint32_t run0 = BG_RUN_BASE (uint32_t)((uint64_t)blockIdx.x * n_runs / gridDim.x);
    const uint32_t run1 = BG_RUN_BASE (uint32_t)((uint64_t)(blockIdx.x + 1) * n_runs / gridDim.x);

    for (int t0 = 0; t0 < n; t0 += tile_cap) {
        const int cnt = std::min(tile_cap, n - t0), cnt4 = (cnt + 3) & ~3;
        __syncthreads();   // the previous tile's counters are out
        for (int i = tid; i < cnt4; i += kThreads) tile[i] = words[t0 + std::min(i, cnt - 1)];   // pad: repeats
        for (int i = tid; i < 2 * cnt4; i += kThreads) scnt[i] = 0u;
        for (uint32_t run = run0; run < run1; ++run) {
            const uint32_t r0 = run * kRun;   // n_runs * kRun <= 2^32: the last run's r0 fits
            __syncthreads();                  // the previous run's windows are cut (and the tile is staged)
            if (tid < kRunWords) {
                const size_t wi = (size_t)(r0 >> 5) + (size_t)tid;
                const uint64_t b = wi < bw ? packed[wi] : 0ull;
                s_lo[tid] = even_bits(b);
                s_hi[tid] = even_bits(b >> 1);
                s_ok[tid] = wi < vw2 ? ok32[wi] : 0u;   // columns past the stream: not bases
            }
            __syncthreads();
            uint2 w[2][kItems];   // [0] the window, [1] its reverse complement
            uint32_t valid = 0;   // bit j: window j holds k bases
#pragma unroll
            for (int j = 0; j < kItems; ++j) {
                const int pl = j * kThreads + tid, i = pl >> 5;
                const uint32_t sh = (uint32_t)(pl & 31);
                const uint32_t lo = __builtin_amdgcn_alignbit(s_lo[i + 1], s_lo[i], sh) & kmask;
                const uint32_t hi = __builtin_amdgcn_alignbit(s_hi[i + 1], s_hi[i], sh) & kmask;
                const uint32_t ok = __builtin_amdgcn_alignbit(s_ok[i + 1], s_ok[i], sh) & kmask;
                valid |= (uint32_t)(ok == kmask) << j;
                w[0][j] = make_word(lo, hi, T());
                w[1][j] = make_word(~(__brev(lo) >> (32 - k)) & kmask, ~(__brev(hi) >> (32 - k)) & kmask, T());
            }
            for (int i = 0; i < cnt4; i += 4) {
                uint2 u[4];
                load4(tile, i, u);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        uint32_t m = 255u;
#pragma unroll
                        for (int j = 0; j < kItems; ++j) m = std::min(m, (uint32_t)__popc(diff_mask(w[s][j], u[q])));
                        if (__any(m <= max_score)) {   // rare: some lane of the wave is within the mismatch count
                            if (i + q < cnt) {
#pragma unroll
                                for (int j = 0; j < kItems; ++j) {
                                    const uint32_t d = diff_mask(w[s][j], u[q]);
                                    const uint32_t pc = (uint32_t)__popc(d);
                                    if (((valid >> j) & 1u) && d <= lim && pc <= max_score) {
                                        atomicAdd(&scnt[2 * (i + q) + s], 1u);
                                        if (LIST) {
                                            const unsigned long long at = atomicAdd(count, 1ull);
                                            if (at < capacity) {
                                                msspe_site rec;
                                                rec.primer = BG_PRIMER_BASE (uint32_t)(t0 + i + q);
                                                rec.pos = r0 + (uint32_t)(j * kThreads + tid);
                                                rec.mismatches = (uint16_t)(pc / (uint32_t)scale);
                                                rec.strand = (uint16_t)s;
                                                sites[at] = rec;
                                            }
                                        }
                                    }
                                }
                            }
                        }
                    }
            }
        }
        __syncthreads();
        for (int i = tid; i < 2 * cnt; i += kThreads) {
            const uint32_t c = scnt[i];
            if (c) atomicAdd(&counts[2 * (size_t)t0 + (size_t)i], (unsigned long long)c);
        }
    }
