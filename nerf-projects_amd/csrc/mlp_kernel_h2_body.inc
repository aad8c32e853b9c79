// The body of nerf_mlp_h2_kernel<MODE, STORE> and of nerf_mlp_h2_fold_kernel<MODE> (mlp_kernel_h2.hip), included into both:
// MODE, STORE and `fold` are compile-time constants of the including kernel, `a` its MlpLaunch, `idle` whether the launch
// belongs to the other kernel (no tile is run then). fold: the view fold
// (nerf_internal.h, PackedNet::d_stream_fold) - feature_linear is not evaluated: the launch reads the folded stream, bias block
// and scales, the trunk's last layer is the pending layer of the view section, and alpha_linear's tile follows the view chunks.
// ray_bias (nerf_mlp_h2_fold_ray_kernel; fold, ray records with a multiple of 32 samples per ray): the view layer's gamma(dir)
// term comes per ray from MlpLaunch::ray_bias instead of being computed per point. kInputRays: a wavefront's 32 points lie on
// one ray, whose row travels through a per-wave LDS slot - see the tile start and the view section. kInputRaysIndexed: the
// listed points of a wavefront lie on any rays, and each lane reads its own ray's entries from the table in the view section.
// (Text, not a function: the static LDS arrays have to be the kernel's own, and with the body behind a function's reference
// and pointer parameters hipcc spilled some hundred registers per lane to scratch.)
    // The ring is the dynamic LDS allocation; the bias block and the small per-layer tables are static.
    extern __shared__ __attribute__((aligned(16))) char ring_lds[];
    __shared__ __attribute__((aligned(16))) float bias_lds[kBiasLdsBytes / 4];
    __shared__ __attribute__((aligned(16))) float layer_tab[4 * (kMaxDepth + 3)];   // per layer [descale, gain, max|b|, -]
    __shared__ unsigned max_record[kBwdMaxSlots];      // STORE: enter_max's records
    __shared__ __attribute__((aligned(16))) float ray_lds[kWavesPerGroup * 256];      // ray_bias: a KiB per wave, its ray's row in front
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5;

    const float* const bias_src = fold ? a.bias_fold : a.bias;
    const float* const descale_src = fold ? a.descale_fold : a.descale;

    FwdPipe pipe{(const char*)(ray_bias ? a.stream_ray : fold ? a.stream_fold : a.stream_h2), ring_lds, 0, wave, lane, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr};
    pipe_start(pipe);
    for (int k = 0; k < 2; ++k) {
        prefetch_pieces<0, 4>(piece_src(pipe, k), piece_dst(pipe, k));
        prefetch_pieces<0, 4>(piece_src(pipe, k) + 4096, piece_dst(pipe, k) + 4096);
    }
    prefetch_pieces<0, 4>(piece_src(pipe, 2), piece_dst(pipe, 2));   // chunk 0's first-half steps issue the other four
    for (int i = threadIdx.x; i < a.n_bias_tiles * kBiasTileFloats; i += 256) bias_lds[i] = bias_src[i];
    if (STORE != 0 && threadIdx.x < kBwdMaxSlots) max_record[threadIdx.x] = threadIdx.x == kBwdMaxGammaD ? 0x3f800000u : 0u;      // (|gamma(d)| <= 1)
    if (threadIdx.x < a.D + 3) {
        const int l = threadIdx.x;
        const bool has_gain = l <= (a.use_viewdirs ? a.D : a.D - 1);
        layer_tab[4 * l] = descale_src[l];
        layer_tab[4 * l + 1] = has_gain ? a.gain[2 * l] : 0.0f;
        layer_tab[4 * l + 2] = has_gain ? a.gain[2 * l + 1] : 0.0f;
        layer_tab[4 * l + 3] = 0.0f;
    }
    __syncthreads();   // chunks 0, 1, the bias block and the layer tables are in LDS
    Frag4 cur;
    {
        const unsigned fr0 = lds_byte_addr(ring_lds) + lane * 16;
        frag_issue<0>(pipe, cur.q[0], fr0);
        frag_issue<1024>(pipe, cur.q[1], fr0);
        frag_issue<2048>(pipe, cur.q[2], fr0);
        frag_issue<3072>(pipe, cur.q[3], fr0);
    }

    const unsigned bias0 = lds_addr(bias_lds) + 64 * h;   // this half-wave's entries of bias-block tile 0
    // kInputRaysIndexed: the tile loop runs over the compacted list, whose length lives on the device (one scalar load); a
    // workgroup without a tile falls through
    int64_t n_live = a.n_points;
    if constexpr (MODE == kInputRaysIndexed) n_live = __builtin_amdgcn_readfirstlane(*a.index_count);
    if (idle) n_live = 0;      // the launch belongs to this kernel's twin
    const int64_t n_tiles = (n_live + kPointsPerGroup - 1) / kPointsPerGroup;
    const int n_layers = (a.use_viewdirs && !fold) ? a.D + 1 : a.D;
    // The tile schedule. Static (a.tile_claim == nullptr; every STORE kernel): workgroup b runs tiles b, b + grid, ... Claimed
    // (tile_claim.h): contiguous batches - the first by position, the later ones from the launch's counter, 15 to 35
    // claims per launch, each in the open at a tile boundary: one lane's returning atomic, handed round through LDS behind
    // one barrier. The bounds are wave-uniform and live in scalar registers. Tile order changes no value.
    __shared__ unsigned claim_lds;
    int64_t tile = blockIdx.x, tile_end = n_tiles;
    int tile_step = gridDim.x, claim_share = 0, claim_done = 0;
    bool claimed = false;
    if constexpr (STORE == 0) claimed = a.tile_claim != nullptr && !idle;
    if (claimed) {
        claim_share = (int)((n_tiles + gridDim.x - 1) / gridDim.x);
        claim_done = tile_claim_batch(claim_share, 0);
        tile = (int64_t)blockIdx.x * claim_done;
        tile_end = tile + claim_done < n_tiles ? tile + claim_done : n_tiles;
        tile_step = 1;
    }
    for (;; tile += tile_step) {
        if (tile >= tile_end) {
            if (!claimed) break;
            const int size = tile_claim_batch(claim_share, claim_done);
            if (threadIdx.x == 0) claim_lds = atomicAdd(a.tile_claim, (unsigned)size);
            __syncthreads();
            tile = (int64_t)gridDim.x * tile_claim_batch(claim_share, 0) +
                   __builtin_amdgcn_readfirstlane(__float_as_uint(lds_scalar((const float*)&claim_lds)));
            if (tile >= n_tiles) break;      // the pool is dry: leave
            tile_end = tile + size < n_tiles ? tile + size : n_tiles;
            claim_done += size;
        }
        pipe_tile_start(pipe);
        const int64_t tile0 = tile * kPointsPerGroup + wave * kPointsPerWave;
        const int64_t pt_raw = tile0 + (lane & 31);
        int64_t pt = pt_raw < n_live ? pt_raw : n_live - 1;
        const int64_t slot = pt;      // STORE: what the backward pass keeps goes to the tile slot - compact, in list order
        if constexpr (MODE == kInputRaysIndexed) pt = a.index[pt];      // the listed point replaces the slot: inputs, output row
        if constexpr (ray_bias && MODE == kInputRays) {
            // This wave's ray (a wave behind the batch's end: the last ray) -> its row of the table into the wave's slot, one
            // LDS-DMA of 64 x 16 bytes (the row has 33 pieces: the lanes behind fetch the last one again). Issued before the
            // tile's first ring piece, so every counted vmcnt(8) of the tile retires it with the pieces before it; the view
            // section, the only reader, is sixty chunks away, and the wave's reads of the previous tile's row have returned
            // (lgkmcnt(0) behind each of them).
            const float* row = a.ray_bias + (pt / a.samples_per_ray) * kRayBiasRow + 4 * (lane < 32 ? lane : 32);
            __builtin_amdgcn_global_load_lds(GLB_PTR(row), LDS_PTR(ray_lds + wave * 256), 16, 0, 0);
        }

        XT xp0, xp1;
        float m_pe;
        int t_pe;
        {
            f32x16 x0, x1, dd;
            load_inputs<MODE, true, false>(a, pt, h, x0, x1, dd);   // gamma(dir) waits for the view layer
            // The ranges of the encoded inputs are taken over the whole wavefront: wave-uniform, so they live in SGPRs
            // (the kernel has no vector register to spare: kept per lane, one of them was spilled to scratch, and its
            // reload - a VMEM load - drained the LDS-DMA weight pipeline with s_waitcnt vmcnt(0) twice per layer).
            // A wave's points share a ray or two, so the common scale costs the split nothing.
            m_pe = wave_max(tile_absmax(x1, tile_absmax(x0, 0.0f)));
            t_pe = pick_exponent(m_pe);
            if constexpr (STORE != 0) enter_max(&max_record[kBwdMaxGammaX], m_pe);      // the gamma(x) columns' weight gradients scale by it
            split_tile(xp0, x0, pow2f(t_pe));
            split_tile(xp1, x1, pow2f(t_pe));
        }

        XT hid[8];
        f32x16 accA[8], accB[8];
        Pending pd;
        float sigma = 0.0f;
        float m_prev = 0.0f;    // largest |activation| of the layer before the pending one... of its inputs

        // what the raw sums of layer l become: called when its chunks are done. m_in = largest |input| of layer l
        // (true units), t_in = exponent its inputs were scaled by
        Tile16 bias0_req;      // bias entries of the pending layer's tile 0, requested by make_pending
        auto make_pending = [&](int l, float m_in, int t_in) {
            const bool is_feature = a.use_viewdirs && l == a.D;
            const bool joins_dir = a.use_viewdirs && l == n_layers - 1;      // feature_linear, or the trunk's last layer when folded
            const unsigned baddr = bias0 + 128 * (is_feature ? 8 * a.D + 1 : 8 * l);
            // the scale-table row and the bias entries of tile 0 in one go: five reads and ONE wait for all of them (one
            // exposed LDS latency per layer instead of two). One statement: with reads still in flight across the
            // arithmetic below, hipcc moved their destination registers whenever that arithmetic changed.
            f32x4 tab;
            asm volatile("ds_read_b128 %0, %5\n\tds_read_b128 %1, %6\n\tds_read_b128 %2, %6 offset:16\n\t"
                         "ds_read_b128 %3, %6 offset:32\n\tds_read_b128 %4, %6 offset:48\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(tab), "=&v"(bias0_req.q[0]), "=&v"(bias0_req.q[1]), "=&v"(bias0_req.q[2]), "=&v"(bias0_req.q[3])
                         : "v"(lds_byte_addr(layer_tab + 4 * l)), "v"(baddr)
                         : "memory");
            pd.c = tab[0] * pow2f(-t_in);
            pd.floor = is_feature ? -__builtin_inff() : 0.0f;
            float bound = fmaf(tab[1], m_in, tab[2]) * 1.001f;
            // the next layer may concatenate these outputs with inputs that must fit the same scale
            if (joins_dir && ray_bias && MODE == kInputRays) {
                // the same number per ray: max(|d|, 1) travels behind the ray's row (kRayBiasMax). It keeps the scale of the trunk
                // output, and with it sigma, bit for bit the folded kernel's.
                bound = fmaxf(bound, lds_scalar(ray_lds + wave * 256 + kRayBiasMax));
            } else if (joins_dir) {
                // range of gamma(dir), which the view layer concatenates: re-read from the ray record here (once per
                // tile) rather than kept in a register through the trunk
                f32x16 x0, x1, dd;
                float m_dd;
                load_inputs<MODE, false, false>(a, pt, h, x0, x1, dd, &m_dd);
                bound = fmaxf(bound, wave_max(m_dd));
            }
            else if ((a.skip_in_mask >> (l + 1)) & 1) bound = fmaxf(bound, m_pe);
            pd.t_out = pick_exponent(bound);
            pd.sc = pow2f(pd.t_out);
            pd.bias_addr = baddr;
            // The running maximum starts at 0 - or at +inf when the layer before had overflowed ON THIS POINT (m_prev = inf; not
            // m_in, which takes in the wave-wide range of the encodings): an activation beyond the fp32 range poisons
            // everything downstream in the reference (F.relu keeps +inf and NaN, nerf.py:72; the next Linear mixes
            // inf - inf), v_max_f32 would quietly drop the NaNs, and carrying the fact in the maximum costs no register:
            // the heads below turn m = inf into the reference's NaN.
            pd.m = fmaxf(m_prev - 3.4028234663852886e38f, 0.0f);
            if constexpr (STORE) {
                pd.maskw = 0u;
                pd.mask_base = wave_uniform(is_feature ? a.st.mask_hv : a.st.mask[l]);      // (feature_linear: not written)
                pd.mask_off = 16u * (2u * (unsigned)slot + (unsigned)h);
                pd.keep_base = (is_feature ? a.st.feat : a.st.h[l]) + (STORE == 2 ? 1024 : 0);      // (blocked: keep_pairs)
                pd.keep_off = 4u * ((unsigned)slot * (unsigned)(is_feature ? a.st.feat_ld : a.st.h_ld[l]) + 4u * (unsigned)h);
                if constexpr (STORE == 2)      // blocked by 32 points: 32 KiB per group of a 256-wide buffer, 32 bytes per point of a piece
                    pd.keep_off = ((unsigned)slot >> 5) * 32768u + ((unsigned)slot & 31u) * 32u + (unsigned)h * 16u;
            }
        };
        // all 8 tiles of the pending layer are converted: its true output range
        auto close_pending = [&](int slot) {
            m_prev = half_max(pd.m);
            if constexpr (STORE) {
                // this layer's ReLU-mask record (for feature_linear, which has no ReLU, the buffer is nullptr-free scratch:
                // see make_pending)
                if (slot != kBwdMaxFeatValue)
                    asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(pd.mask_off), "v"(pd.maskq), "s"(pd.mask_base) : "memory");
                // the largest kept activation of this layer, for the weight-gradient kernel's scale (MlpStore::maxes)
                enter_max(&max_record[slot], m_prev);
            }
            // the scale was chosen for a bound of 2^(10 - t_out); outputs 2^12 and more below it have begun to lose
            // low-half bits (see Pending). Counted, never silent: nerf_precision_status.
            const int slack = 10 - pd.t_out - __builtin_amdgcn_frexp_expf(m_prev);
            if (m_prev > 0.0f && m_prev < __builtin_inff() && slack >= 12 && pd.t_out > -60 && a.loose) atomicAdd(a.loose, 1u);
        };

        // layer 0: gamma(xyz) -> W (nerf.py:70-73)
        chunk_ktile8<-1, true>(pipe, cur, accA, xp0, hid, accB, pd);
        chunk_ktile8<-1, false>(pipe, cur, accA, xp1, hid, accB, pd);
        make_pending(0, m_pe, t_pe);

        // trunk layers 1..D-1, then (with viewdirs) feature_linear as layer D without ReLU. Layer l accumulates
        // into `out` while the pending layer l-1 is converted out of `pend`.
        auto layer_pass = [&](f32x16 (&pend)[8], f32x16 (&out)[8], int l) {
            convert_tile0_with<STORE>(hid[0], pend[0], pd, bias0_req);
            chunk_ktile8<1, true, STORE>(pipe, cur, out, hid[0], hid, pend, pd);
            next_tile_pair<STORE>(pd);
            chunk_ktile8<2, false, STORE>(pipe, cur, out, hid[1], hid, pend, pd);
            chunk_ktile8<3, false, STORE>(pipe, cur, out, hid[2], hid, pend, pd);
            next_tile_pair<STORE>(pd);
            chunk_ktile8<4, false, STORE>(pipe, cur, out, hid[3], hid, pend, pd);
            chunk_ktile8<5, false, STORE>(pipe, cur, out, hid[4], hid, pend, pd);
            next_tile_pair<STORE>(pd);
            chunk_ktile8<6, false, STORE>(pipe, cur, out, hid[5], hid, pend, pd);
            chunk_ktile8<7, false, STORE>(pipe, cur, out, hid[6], hid, pend, pd);
            chunk_ktile8<-1, false>(pipe, cur, out, hid[7], hid, pend, pd);
            close_pending(kBwdMaxKept + l - 1);
            const int t_in = pd.t_out;
            float m_in = m_prev;
            if (a.use_viewdirs && l == a.D) {
                // alpha_linear reads the post-ReLU trunk output (nerf.py:86), i.e. this layer's input: one more
                // chunk, a single-row tile accumulated into a pending tile that is no longer needed
                chunk_row8(pipe, cur, pend[0], hid);
                sigma = fmaf(pend[0][0], lds_scalar(layer_tab + 4 * (a.D + 2)) * pow2f(-t_in), lds_scalar(bias_lds + (8 * a.D) * 32));
                if (!(m_prev < __builtin_inff())) sigma = __builtin_nanf("");      // the trunk overflowed on this point (make_pending)
            }
            if (!(a.use_viewdirs && l == a.D) && ((a.skip_in_mask >> l) & 1)) {
                // h = cat[input_pts, h] (nerf.py:79-80): bring the encoded inputs to this layer's scale
                rescale_tile(xp0, t_in - t_pe);
                rescale_tile(xp1, t_in - t_pe);
                t_pe = t_in;
                chunk_ktile8<-1, false>(pipe, cur, out, xp0, hid, pend, pd);
                chunk_ktile8<-1, false>(pipe, cur, out, xp1, hid, pend, pd);
                m_in = fmaxf(m_in, m_pe);
            }
            make_pending(l, m_in, t_in);
        };
        int l = 1;
        bool pend_in_a = true;
        while (l < n_layers) {
            layer_pass(accA, accB, l);
            ++l;
            pend_in_a = false;
            if (l >= n_layers) break;
            layer_pass(accB, accA, l);
            ++l;
            pend_in_a = true;
        }
        if (!pend_in_a) {
#pragma unroll
            for (int t = 0; t < 8; ++t) accA[t] = accB[t];
        }

        const bool live = pt_raw < n_live;
        if (a.use_viewdirs) {
            // views_linears[0] on cat[feature, gamma(dir)] (nerf.py:93-98): 4 output tiles; the pending layer is
            // feature_linear - or, folded, the trunk's last layer, which the folded matrix reads directly
            convert_tile0_with<STORE>(hid[0], accA[0], pd, bias0_req);
            convert_tile<1, STORE>(hid[1], accA[1], pd);
            next_tile_pair<STORE>(pd);
            chunk_pair4<2, true, STORE>(pipe, cur, accB, hid[0], hid[1], hid, accA, pd);
            next_tile_pair<STORE>(pd);
            chunk_pair4<4, false, STORE>(pipe, cur, accB, hid[2], hid[3], hid, accA, pd);
            next_tile_pair<STORE>(pd);
            chunk_pair4<6, false, STORE>(pipe, cur, accB, hid[4], hid[5], hid, accA, pd);
            chunk_pair4<-1, false>(pipe, cur, accB, hid[6], hid[7], hid, accA, pd);
            close_pending(kBwdMaxFeatValue);
            const bool rgb_poisoned = !(m_prev < __builtin_inff());      // the trunk or feature_linear overflowed (make_pending)
            if constexpr (fold) {
                // alpha_linear on the trunk output (nerf.py:86), all of which is converted only now: its tile accumulates into
                // a pending tile that is no longer needed, at the scale layer_pass uses in the unfolded order
                chunk_row8(pipe, cur, accA[0], hid);
                sigma = fmaf(accA[0][0], lds_scalar(layer_tab + 4 * (a.D + 2)) * pow2f(-pd.t_out), lds_scalar(bias_lds + (8 * a.D) * 32));
                if (rgb_poisoned) sigma = __builtin_nanf("");      // the trunk overflowed on this point
                // The reference forms the feature vector, and one that overflows fp32 poisons the colours; here it never exists.
                // Its a-priori bound (feature_linear's gain pair) says whether it could have: not provably finite on a finite
                // trunk output = one loose-bound event, and the guard's fp32 pass settles it (DESIGN 8). Eligibility
                // (view_fold_eligible_kernel) keeps this to trunk outputs beyond 2^64. One event per point: m_prev is the
                // point's (half_max), and the lower half-wave's lane counts it - a live one: the slots behind the batch's end
                // evaluate its last point again and must not count it again.
                const float feat_bound = fmaf(lds_scalar(layer_tab + 4 * a.D + 1), m_prev, lds_scalar(layer_tab + 4 * a.D + 2));
                if (h == 0 && live && !rgb_poisoned && !(feat_bound < __builtin_inff()) && a.loose) atomicAdd(a.loose, 1u);
            }
            if constexpr (!ray_bias) {      // (ray_bias: the term is in the ray's row, the stream has no gamma(dir) chunk)
                XT xd;
                {
                    f32x16 x0, x1, dd;
                    load_inputs<MODE, false, true>(a, pt, h, x0, x1, dd);
                    split_tile(xd, dd, pd.sc);
                }
                chunk_ktile4(pipe, cur, accB, xd);
            }
            unsigned bad;     // raw inputs re-read (a value kept across the view layer costs the step a register): requested
            {                 // here, behind the last MFMA chunk, so that the round trip runs under the colour head's arithmetic
                f32x16 x0, x1, dd;
                load_inputs<MODE, false, false>(a, pt, h, x0, x1, dd, nullptr, &bad);
            }
            f32x16 y[4];
            // (ray_bias: b_vf + W_v[:, W:] gamma(dir) of the wave's ray, in the order of the bias tiles it stands in for)
            if constexpr (ray_bias && MODE == kInputRaysIndexed)      // (the same entries, each lane's from its own ray's row)
                finish_views_row(y, accB, a.ray_bias + (pt / a.samples_per_ray) * kRayBiasRow + 16 * h,
                                 lds_scalar(layer_tab + 4 * (a.D + 1)) * pow2f(-pd.t_out));
            else
                finish_views(y, accB, ray_bias ? lds_addr(ray_lds + wave * 256) + 64 * h : bias0 + 128 * (8 * a.D + 9),
                             lds_scalar(layer_tab + 4 * (a.D + 1)) * pow2f(-pd.t_out));
            if constexpr (STORE) {
                const unsigned off = 4u * ((unsigned)slot * (unsigned)a.st.hv_ld + 4u * (unsigned)h);
                keep_tiles4<0>(a.st.hv, off, y);
                // the view layer's ReLU mask in the bit order of the trunk layers' (MlpStore::mask_hv, words 0 and 1)
                const unsigned moff = 16u * (2u * (unsigned)slot + (unsigned)h);
                const u32x4 rec = {relu_mask_word(y[0], y[1]), relu_mask_word(y[2], y[3]), 0u, 0u};
                asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(moff), "v"(rec), "s"(a.st.mask_hv) : "memory");
            }
            // rgb_linear (nerf.py:101): three rows over the 128-wide view layer
            const float* rb = bias_lds + (8 * a.D + 13) * 32;
            const float r0 = row_dot4(y, bias0 + 128 * (8 * a.D + 22)) + lds_scalar(rb);
            const float r1 = row_dot4(y, bias0 + 128 * (8 * a.D + 26)) + lds_scalar(rb + 1);
            const float r2 = row_dot4(y, bias0 + 128 * (8 * a.D + 30)) + lds_scalar(rb + 2);
            if (MODE == kInputLattice) {
                // the density lattice keeps sigma alone: relu(raw[..., 3]) (nerf.ipynb:291)
                if (live && h == 0) a.out[pt] = relu_keep_nan((bad & kBadXyz) ? __builtin_nanf("") : sigma);
            } else if (live && h == 0) {
                f32x4 o = {r0, r1, r2, sigma};   // outputs = cat[rgb, alpha] (nerf.py:106)
                if (bad || rgb_poisoned) {       // NaN / Inf inputs propagate as through F.relu (see kBadXyz)
                    const float qnan = __builtin_nanf("");
                    o = f32x4{qnan, qnan, qnan, (bad & kBadXyz) ? qnan : sigma};
                }
                *(f32x4*)(a.out + pt * 4) = o;
            }
        } else {
            // output_linear (nerf.py:109): rows 0..out_ch-1 of one tile; the pending layer is trunk layer D-1 (STORE: kept, with
            // its mask record and maximum, like every other trunk layer - the training pass of networks without view directions)
            convert_tile0_with<STORE>(hid[0], accA[0], pd, bias0_req);
            convert_tile<1, STORE>(hid[1], accA[1], pd);
            next_tile_pair<STORE>(pd);
            convert_tile<2, STORE>(hid[2], accA[2], pd);
            convert_tile<3, STORE>(hid[3], accA[3], pd);
            next_tile_pair<STORE>(pd);
            convert_tile<4, STORE>(hid[4], accA[4], pd);
            convert_tile<5, STORE>(hid[5], accA[5], pd);
            next_tile_pair<STORE>(pd);
            convert_tile<6, STORE>(hid[6], accA[6], pd);
            convert_tile<7, STORE>(hid[7], accA[7], pd);
            if constexpr (STORE != 0) close_pending(kBwdMaxKept + a.D - 1);
            const bool poisoned = !(half_max(pd.m) < __builtin_inff());      // the trunk overflowed on this point (make_pending)
            f32x16 o;
            chunk_row8(pipe, cur, o, hid);
            Tile16 b = lds_tile_issue(bias0 + 128 * (8 * a.D));
            lds_tile_wait(b);
            const float c = lds_scalar(layer_tab + 4 * a.D) * pow2f(-pd.t_out);
            unsigned bad;
            {
                f32x16 x0, x1, dd;
                load_inputs<MODE, false, false>(a, pt, h, x0, x1, dd, nullptr, &bad);
            }
            if (live) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float v = ((bad & kBadXyz) || poisoned) ? __builtin_nanf("") : fmaf(o[r], c, b.q[r >> 2][r & 3]);
                    if (MODE == kInputLattice) {
                        if (row == 3) a.out[pt] = relu_keep_nan(v);      // sigma alone (nerf.ipynb:291)
                    } else if (row < a.out_ch) {
                        a.out[pt * a.out_ch + row] = v;
                    }
                }
            }
        }
    }   // tile loop
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (claimed && threadIdx.x == 0) {
        // every workgroup of the launch passes here once, behind its last claim: the last one out zeroes the counter and the
        // count of leavers for the next launch in the stream
        if (atomicAdd(a.tile_claim + 1, 1u) == gridDim.x - 1) {
            __hip_atomic_store(a.tile_claim, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.tile_claim + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (STORE) {
        __syncthreads();
        flush_maxes(a.st.maxes, max_record, kBwdMaxSlots);
    }
