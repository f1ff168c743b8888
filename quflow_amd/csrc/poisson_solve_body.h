// The body of the chunked Thomas solve, included by poisson.hip once per kernel: k_solve<R, L, SKEWH, FOLD> with
// QF_SOLVE_OFFSET 0, k_solve_off<L, FOLD> (R = double, SKEWH = 1) with QF_SOLVE_OFFSET 1 and the extra argument F.
// QF_SOLVE_OFFSET 1: the right-hand side is W - F, F an N x N matrix read entry by entry next to W in the same walk -- the
// arithmetic of solve(W - F).  Everything behind the load (trace removal, sweeps, mirror, both FOLD layouts) sees v[] only.
// The skew-Hermitian solve reads the upper triangle of its right-hand side alone, so F must be exactly skew-Hermitian
// (checked where it is installed).
// Text, not an inlined function template: through a __forceinline__ template the plain kernels came out of the code
// generator with other register counts (16 of the 20 instantiations) -- included text leaves them bit for bit.
// Expects in scope: R, L, SKEWH, FOLD; N, G, C, W, P, tab, scale, guard, dec, tail_off (and F).
{
#if QF_SOLVE_OFFSET
    typedef double R;
    constexpr int SKEWH = 1;
#endif
    typedef typename rt<R>::C cplx;      // (shadows the file-level double2 typedef inside the kernel)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // Deferred step end: the second product before this launch left its row sums and
    // qf_dev_state::pending.  Every workgroup forms the decision itself and acts on it at once; thread 0 takes a
    // ticket whose answer is looked at when the workgroup is done: the last arrival (everyone else has read the old
    // state by then) writes the new state and publishes the progress.
    // (Tried: issuing this thread's loads from BOTH Whalf candidates and its table loads first and forming the
    // decision while they travel -- 8,745 against 9,137 timesteps/s at N = 512: twice the sweep loads and 70 more
    // registers cost more than the hidden round trip saved.)
    qf_new_state ns;
    bool decided = false;
    unsigned my_ticket = 0u;
    if (dec.state_rw) {
        // (in this protocol practically every solve follows a second product: the row sums are requested at once,
        // together with the control state, not behind the look at `pending` -- one memory round trip, not two)
        ns = qf_decide_compute(N, dec.slots, dec.rowpart, dec.state_rw, reinterpret_cast<double *>(smem_raw));
        if (dec.state_rw->pending) {
            decided = true;
            if (threadIdx.x == 0) my_ticket = __hip_atomic_fetch_add(dec.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#define QF_SOLVE_EXIT                                                                           \
    {                                                                                           \
        if (decided && threadIdx.x == 0 && my_ticket == gridDim.x - 1) qf_decide_apply(dec.state_rw, dec.rec, dec.ticket, ns); \
    }
    const int tid = threadIdx.x;
    const int nthreads = blockDim.x;  // = G*C rounded up to a multiple of 64
    const int lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
    const int g = tid % G;
    const int jc = tid / G;           // chunk index (>= C for padding threads)
    // workgroup -> walk group, XCD-aware: consecutive workgroup ids go
    // round-robin over the 8 XCDs; neighbouring walk groups share their 128-byte lines (G = 4 walks
    // are 64 bytes of a row), so XCD x takes a contiguous range of walk groups
    int bid = blockIdx.x;
    {
        const int nb = gridDim.x, slot = bid & 7, l = bid >> 3;
        int start = 0;
        for (int y = 0; y < slot; ++y) start += (nb - y + 7) >> 3;
        bid = start + l;
    }
    const int t0 = bid * G;
    const int t = t0 + g;
    const int T = FOLD ? (N + 1) / 2 : (SKEWH ? N : N + 1);
    const size_t NN = (size_t)N * N;
    const size_t stride = (size_t)N + 1;
    // one wavefront scans the chunk carries of a walk: one chunk per lane up to 64 chunks, two up to 128
    const bool use_scan = (C <= 128);
    const bool scan_pairs = (C > 64);

    // LDS carve-up (scan phase): endv[C*G] complex, carry[C*G] complex, red[nthreads] complex,
    // endc[C*G] real.  The mirror staging tile ptile[C*L][G] reuses the same memory afterwards.
    // The chunk-end records are written chunk-by-thread (lanes run over the G walks fastest) and read walk-major
    // by the scan (lanes run over the chunks), the carries the other way round: each is a transposition through
    // LDS.  Padded strides keep both sides conflict-free (round 2's unpadded layout had 4-way conflicts on the
    // strided side: SQ_LDS_BANK_CONFLICT = 50 % of the kernel's LDS cycles): walk stride C + 2 complex entries
    // (G walks x 2 chunks of a b128 lane group land in 8 distinct 4-bank slots), C + 4 reals for the products,
    // G + 1 complex entries per chunk row of the carries.
    const int CE = C + 2, CR = C + 4, GP = G + 1;
    cplx *endv = reinterpret_cast<cplx *>(smem_raw);
    cplx *carry = endv + (size_t)CE * G;
    cplx *red = carry + (size_t)C * GP;
    R *endc = reinterpret_cast<R *>(red + nthreads);
    cplx *ptile = reinterpret_cast<cplx *>(smem_raw);
    cplx *red2 = reinterpret_cast<cplx *>(smem_raw + tail_off);   // 8 entries behind the larger of the two carve-ups
    // chunk-end records: walk-major for the wavefront scan, chunk-major for the serial pass
    const int end_idx = use_scan ? g * CE + jc : jc * G + g;
    const int endc_idx = use_scan ? g * CR + jc : jc * G + g;

    QF_PROBE_STAMP(0)
    int len = 0;
    if (t < T && jc < C) len = SKEWH ? (N - t) : (int)((NN - 1 - (size_t)t) / stride) + 1;
    // FOLD: len1 entries of walk t, then len2 of walk t2 = N-1-t (none when that is walk t itself: odd N's middle)
    const int len1 = len;
    const int t2 = N - 1 - t;
    if (FOLD && len > 0 && t2 != t) len += t + 1;
    // entry k of the sequence lives at base(k) + k * stride
    const long long base1 = t, base2 = (long long)t2 - (long long)len1 * (long long)stride;
    const bool has_trace = (bid == 0);  // the block that owns walk t = 0 (m = 0)
    const bool on_diag = (t == 0 && jc < C);   // (FOLD: for the entries k < len1 of this slot)

    const int k0 = jc * L;
    const size_t e0 = (size_t)t + (size_t)k0 * stride;
#define QF_ENTRY(k_) (FOLD ? (size_t)((((k_) < len1) ? base1 : base2) + (long long)(k_) * (long long)stride) : e0 + (size_t)((k_) - k0) * stride)

    cplx v[L];
    R w[L + 1];
    R inv[L];

    // ---- all global loads of this thread are issued up front and unconditionally (invalid
    // steps read a harmless in-range entry and are masked afterwards): a predicated load sits
    // behind a branch, which would serialise 3*L memory round trips behind the FMA chain.
    // Round 4: the factor table is data independent and nobody writes it -- its L + 1 loads go out BEFORE the tag
    // look-up below (the control state was last written by another XCD: its scalar loads are a memory round trip,
    // during which the table entries now travel; a launch that is not due drops them).  The deferred decision of the
    // small sizes stays ahead of them: everything waits for it, and loads return in order (with the table loads in
    // front of it N = 512 lost 0.5 %).
    // (the 32-entry chunks of the largest sizes keep the old order: their 256 + 100 registers leave no room for it)
    constexpr bool EARLY_TAB = (L <= 17);
    const size_t e_safe = (t < T) ? (size_t)t : 0;
    if constexpr (EARLY_TAB) {
#pragma unroll
        for (int s = 0; s < L; ++s) {
            const bool valid = (k0 + s) < len;
            const size_t e = valid ? QF_ENTRY(k0 + s) : e_safe;
            const cplx tb = tab[e];
            w[s] = tb.x;
            inv[s] = tb.y;
        }
        const bool valid = (k0 + L) < len;
        w[L] = tab[valid ? QF_ENTRY(k0 + L) : e_safe].x;
        if (!valid) w[L] = R(0);   // also the multiplier that links to the next chunk (backward sweep)
    }
    {
        bool due = true;
        int wh_sel = 0;
        if (decided) {
            due = (ns.step_index == guard.step && ns.iters_this_step == guard.iter);
            wh_sel = ns.wh_sel;
        } else if (guard.state) {
            due = qf_guard_iter(guard);       // tagged stepper launch that is not due: no-op
            wh_sel = guard.state->wh_sel;
        }
        if (!due) {
            QF_SOLVE_EXIT
            return;
        }
        // fused step end: the first iteration of a step reads the Whalf the previous step's last
        // product prepared for it (uniform scalar decision)
        if (guard.alt && wh_sel) W = static_cast<const cplx *>(guard.alt);
    }
#pragma unroll
    for (int s = 0; s < L; ++s) {
        const bool valid = (k0 + s) < len;
        const size_t e = valid ? QF_ENTRY(k0 + s) : e_safe;
        v[s] = W[e];          // (nontemporal loads here were tried: 30.7 us instead of 21.4)
#if QF_SOLVE_OFFSET
        {
            const cplx f = F[e];      // the offset travels with W: the same walk, the same entry
            v[s].x -= f.x;
            v[s].y -= f.y;
        }
#endif
        if constexpr (!EARLY_TAB) {
            const cplx tb = tab[e];
            w[s] = tb.x;
            inv[s] = tb.y;
        }
    }
    if constexpr (!EARLY_TAB) {
        const bool valid = (k0 + L) < len;
        w[L] = tab[valid ? QF_ENTRY(k0 + L) : e_safe].x;
        if (!valid) w[L] = R(0);
    }
    // ---- m = 0: circulation tr(W)/N, cpu.py:311-317.  The diagonal IS walk 0: its entries are already in the
    // registers of this workgroup's g = 0 threads (rounds 1-4 loaded them a second time, in a loop of dependent
    // round trips behind the sweep loads: the workgroup that owns walk 0 -- the longest walks of the launch --
    // ended last by that much).  One barrier: nobody writes red[] again before the tr(P) sum, which has its own.
    cplx trW = mkc<R>(R(0), R(0));
    if (has_trace && !QF_PROBE_SKIP(2)) {
        cplx s = mkc<R>(R(0), R(0));
        if (on_diag) {
#pragma unroll
            for (int q = 0; q < L; ++q) {
                if ((k0 + q) < len1) {
                    s.x += v[q].x;
                    s.y += v[q].y;
                }
            }
        }
        block_sum_post<R>(s, red, tid);
        __syncthreads();
        s = block_sum_read<R>(red, nthreads);
        R invN = R(1) / (R)N;
        trW = mkc<R>(s.x * invN, s.y * invN);
    }

#pragma unroll
    for (int s = 0; s < L; ++s) {
        const bool valid = (k0 + s) < len;
        if (!valid) {
            v[s] = mkc<R>(R(0), R(0));
            w[s] = R(0);
            inv[s] = R(0);
        } else if (on_diag && (!FOLD || (k0 + s) < len1)) {
            v[s].x -= trW.x;
            v[s].y -= trW.y;
        }
    }

    QF_PROBE_STAMP(1)
    // ---- pass 1: local forward sweep with zero carry-in
    {
        cplx yprev = mkc<R>(R(0), R(0));
        R cprod = R(1);
#pragma unroll
        for (int s = 0; s < L; ++s) {
            cplx y;
            y.x = fma_r(-w[s], yprev.x, v[s].x);
            y.y = fma_r(-w[s], yprev.y, v[s].y);
            v[s] = y;
            cprod *= -w[s];
            yprev = y;
        }
        if (jc < C) {
            endv[end_idx] = yprev;
            endc[endc_idx] = cprod;
        }
    }
    QF_PROBE_STAMP(2)
    __syncthreads();
    QF_PROBE_STAMP(3)

    // ---- pass 2: chunk carries of the forward recurrence
    if (use_scan && scan_pairs) {
        // lane l composes the maps of chunks 2l and 2l+1, the wavefront scans the 64 compositions, and the
        // second chunk's carry is the first one's map applied to the lane's
        for (int gd = wave; gd < G; gd += nwaves) {
            const int c0 = 2 * lane, c1 = c0 + 1;
            R a0 = R(0), a1 = R(0);
            cplx b0 = mkc<R>(R(0), R(0)), b1 = b0;
            if (c0 < C) {
                a0 = endc[gd * CR + c0];
                b0 = endv[gd * CE + c0];
            }
            if (c1 < C) {
                a1 = endc[gd * CR + c1];
                b1 = endv[gd * CE + c1];
            }
            R a = a1 * a0;
            cplx b = mkc<R>(fma_r(a1, b0.x, b1.x), fma_r(a1, b0.y, b1.y));
            scan_affine(a, b, lane, 64);
            R cx = lane_before(b.x), cy = lane_before(b.y);
            if (lane == 0) cx = cy = R(0);
            if (c0 < C) carry[c0 * GP + gd] = mkc<R>(cx, cy);
            if (c1 < C) carry[c1 * GP + gd] = mkc<R>(fma_r(a0, cx, b0.x), fma_r(a0, cy, b0.y));
        }
    } else if (use_scan) {
        if (C > 32) scan_chunks<R, 64, false>(C, G, CE, CR, GP, endc, endv, carry, lane, wave, nwaves);
        else scan_chunks<R, 0, false>(C, G, CE, CR, GP, endc, endv, carry, lane, wave, nwaves);
    } else if (tid < G) {
        cplx c = mkc<R>(R(0), R(0));
        for (int q = 0; q < C; ++q) {
            carry[q * GP + tid] = c;
            cplx ev = endv[q * G + tid];
            R ec = endc[q * G + tid];
            c.x = fma_r(ec, c.x, ev.x);
            c.y = fma_r(ec, c.y, ev.y);
        }
    }
    QF_PROBE_STAMP(4)
    __syncthreads();
    QF_PROBE_STAMP(5)

    // ---- pass 3: apply the carry, normalise by the pivot:  c_k = y_k / b'_k
    {
        cplx corr = mkc<R>(R(0), R(0));
        if (jc < C) corr = carry[jc * GP + g];
#pragma unroll
        for (int s = 0; s < L; ++s) {
            corr.x *= -w[s];
            corr.y *= -w[s];
            v[s].x = (v[s].x + corr.x) * inv[s];
            v[s].y = (v[s].y + corr.y) * inv[s];
        }
    }

    // ---- pass 4: local backward sweep with zero carry-in:  p_k = c_k - w_{k+1} p_{k+1}
    {
        cplx pnext = mkc<R>(R(0), R(0));
        R dprod = R(1);
#pragma unroll
        for (int s = L - 1; s >= 0; --s) {
            cplx p;
            p.x = fma_r(-w[s + 1], pnext.x, v[s].x);
            p.y = fma_r(-w[s + 1], pnext.y, v[s].y);
            v[s] = p;
            dprod *= -w[s + 1];
            pnext = p;
        }
        __syncthreads();  // every thread has consumed carry[] / endv[] of the forward pass
        if (jc < C) {
            endv[end_idx] = pnext;
            endc[endc_idx] = dprod;
        }
    }
    QF_PROBE_STAMP(6)
    __syncthreads();
    QF_PROBE_STAMP(7)

    // ---- pass 5: chunk carries of the backward recurrence (chunks in reverse order)
    if (use_scan && scan_pairs) {
        for (int gd = wave; gd < G; gd += nwaves) {
            const int c0 = C - 1 - 2 * lane, c1 = c0 - 1;     // (reverse order: c0 is met first)
            R a0 = R(0), a1 = R(0);
            cplx b0 = mkc<R>(R(0), R(0)), b1 = b0;
            if (c0 >= 0) {
                a0 = endc[gd * CR + c0];
                b0 = endv[gd * CE + c0];
            }
            if (c1 >= 0) {
                a1 = endc[gd * CR + c1];
                b1 = endv[gd * CE + c1];
            }
            R a = a1 * a0;
            cplx b = mkc<R>(fma_r(a1, b0.x, b1.x), fma_r(a1, b0.y, b1.y));
            scan_affine(a, b, lane, 64);
            R cx = lane_before(b.x), cy = lane_before(b.y);
            if (lane == 0) cx = cy = R(0);
            if (c0 >= 0) carry[c0 * GP + gd] = mkc<R>(cx, cy);
            if (c1 >= 0) carry[c1 * GP + gd] = mkc<R>(fma_r(a0, cx, b0.x), fma_r(a0, cy, b0.y));
        }
    } else if (use_scan) {
        if (C > 32) scan_chunks<R, 64, true>(C, G, CE, CR, GP, endc, endv, carry, lane, wave, nwaves);
        else scan_chunks<R, 0, true>(C, G, CE, CR, GP, endc, endv, carry, lane, wave, nwaves);
    } else if (tid < G) {
        cplx c = mkc<R>(R(0), R(0));
        for (int q = C - 1; q >= 0; --q) {
            carry[q * GP + tid] = c;
            cplx ev = endv[q * G + tid];
            R ec = endc[q * G + tid];
            c.x = fma_r(ec, c.x, ev.x);
            c.y = fma_r(ec, c.y, ev.y);
        }
    }
    QF_PROBE_STAMP(8)
    __syncthreads();
    QF_PROBE_STAMP(9)

    // ---- pass 6: apply the carry
    {
        cplx corr = mkc<R>(R(0), R(0));
        if (jc < C) corr = carry[jc * GP + g];
#pragma unroll
        for (int s = L - 1; s >= 0; --s) {
            corr.x *= -w[s + 1];
            corr.y *= -w[s + 1];
            v[s].x += corr.x;
            v[s].y += corr.y;
        }
    }

    // ---- m = 0: remove tr(P)/N, cpu.py:342-352.  The wave totals go to red2[] behind everything else in LDS (the
    // staging tile overlays red[]), and the barrier between posting and reading them is the one the staging tile
    // needs anyway: the workgroup that owns walk 0 passes no barrier the others do not
    const bool with_trace = has_trace && !QF_PROBE_SKIP(2);
    if (with_trace) {
        cplx s = mkc<R>(R(0), R(0));
        if (on_diag) {
#pragma unroll
            for (int q = 0; q < L; ++q) {
                if ((k0 + q) < len1) {
                    s.x += v[q].x;
                    s.y += v[q].y;
                }
            }
        }
        block_sum_post<R>(s, red2, tid);
    }

    QF_PROBE_STAMP(10)
    // ---- store (scaled); stage the block's results for the mirrored store
    if (SKEWH || with_trace) __syncthreads();  // carry[] is dead: its memory becomes the staging tile
    if (with_trace && on_diag) {
        const cplx s = block_sum_read<R>(red2, nthreads);
        R invN = R(1) / (R)N;
        R tx = s.x * invN, ty = s.y * invN;
#pragma unroll
        for (int q = 0; q < L; ++q) {
            if (!FOLD || (k0 + q) < len1) {
                v[q].x -= tx;
                v[q].y -= ty;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < L; ++s) {
        const int k = k0 + s;
        cplx p = mkc<R>(v[s].x * scale, v[s].y * scale);
        if (k < len && !QF_PROBE_SKIP(0)) P[QF_ENTRY(k)] = p;
        // (walk-per-slot layout: L * G entries between two chunks are a multiple of 256 bytes -- the four chunks of
        // a 16-lane group would write the same banks; G entries of padding per chunk put them 64 bytes apart.  The
        // folded layout's odd L does that by itself.)
        if (SKEWH && jc < C) ptile[(size_t)(FOLD ? k : k + jc) * G + g] = p;
    }
#undef QF_ENTRY
    if (SKEWH && FOLD) {
        // the mirror of both halves: walks t0+gg (entries k of the slot, target row t0 + u with u = k + gg, columns
        // u .. u-G+1) and walks N-1-t0-gg (entries k' behind the slot's first len1; target row N-1-t0 + u' with
        // u' = k' - gg, columns u' .. u'+G-1): contiguous 16*G-byte row segments either way
        __syncthreads();
        const int gg = tid % G, uu = tid / G, upb = nthreads / G;
        const int tt = t0 + gg;
        const int l1 = (tt < T) ? N - tt : 0;
        const int l2 = (tt < T && N - 1 - tt != tt) ? tt + 1 : 0;
        if (!QF_PROBE_SKIP(1)) {
            const int umax = N - t0 + G - 1;
            if (tt != 0) {
                for (int u0 = uu; u0 < umax; u0 += 4 * upb) {
                    cplx p[4];
                    bool ok[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int u = u0 + q * upb, k = u - gg;
                        ok[q] = (u < umax && k >= 0 && k < l1);
                        p[q] = ptile[(size_t)(ok[q] ? k : 0) * G + gg];
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int u = u0 + q * upb, k = u - gg;
                        if (ok[q]) P[(size_t)(t0 + u) * N + k] = mkc<R>(-p[q].x, p[q].y);
                    }
                }
            }
            const int vmax = t0 + G;              // v = u' + G - 1 = 0 .. t0 + G - 1
            for (int v0 = uu; v0 < vmax; v0 += 4 * upb) {
                cplx p[4];
                bool ok[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int kk = v0 + q * upb - (G - 1) + gg;
                    ok[q] = (v0 + q * upb < vmax && kk >= 0 && kk < l2);
                    p[q] = ptile[(size_t)(ok[q] ? l1 + kk : 0) * G + gg];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int up = v0 + q * upb - (G - 1), kk = up + gg;
                    if (ok[q]) P[(size_t)(N - 1 - t0 + up) * N + kk] = mkc<R>(-p[q].x, p[q].y);
                }
            }
        }
    } else if (SKEWH) {
        QF_PROBE_STAMP(11)
        // (i,j) = (k, k+t)  ->  P[j,i] = -conj(P[i,j]), cpu.py:334,340.  With u = k + g the
        // targets of a fixed u are row t0+u, columns u, u-1, .., u-G+1: one contiguous segment.
        __syncthreads();
        const int gg = tid % G, uu = tid / G, upb = nthreads / G;
        const int tt = t0 + gg;
        const int lent = (tt < N) ? N - tt : 0;
        // (k < N - tt means u = k + gg < N - t0: no row beyond that has an entry -- at N = 512 the walk-0 workgroup,
        // which ends last, makes two trips of 256 rows instead of three)
        const int umax = min(C * L + G - 1, N - t0);
        if (tt != 0 && !QF_PROBE_SKIP(1)) {
            // four rows per trip: the LDS reads of a trip are in flight together, then its stores
            for (int u0 = uu; u0 < umax; u0 += 4 * upb) {
                cplx p[4];
                bool ok[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int u = u0 + q * upb, k = u - gg;
                    ok[q] = (u < umax && k >= 0 && k < lent);
                    p[q] = ptile[(size_t)(ok[q] ? k + k / L : 0) * G + gg];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int u = u0 + q * upb, k = u - gg;
                    if (ok[q]) P[(size_t)(t0 + u) * N + k] = mkc<R>(-p[q].x, p[q].y);
                }
            }
        }
    }
    QF_PROBE_STAMP(12)
    QF_SOLVE_EXIT
#undef QF_SOLVE_EXIT
}
