// After an optimiser step: everything the fp16-pair kernels read, rebuilt from the row-equalised parameters in TWO launches.
//
// The training step changes the master parameters once per iteration (nerf.ipynb:1275, optimizer.step()); the fused kernels read
// packed derivatives of them: per network the forward weight stream (fp32 -> fp16 pairs, one power-of-two scale per layer), the
// bias block, the per-layer gains that bound a layer's outputs, and - for the backward-data kernel - the transposed-weight
// stream with its scales and gains. Stage by stage that was 11 launches per network and direction (gathers, per-chunk maxima,
// conversions, a copy of the stream's head behind its end, memsets, gains: api.cpp refresh_h2_many, train_api.cpp
// refresh_bwd - which remain, for loading and for the first use of a stream). Here:
//   refresh_gather_kernel    every stream's chunks gathered through their index tables with the chunk's largest |w| found on the
//                            way (gather_kernel + chunk_absmax_kernel), the bias blocks gathered, the gain tables zeroed
//   refresh_convert_kernel   every chunk split into fp16 (hi, lo) pairs at its layer's scale (convert_stream_h2_kernel, incl.
//                            the copy of a stream's first chunks behind its end), the forward and backward gains
//                            (layer_gain_kernel, layer_gain_bwd_kernel), and the precision guard's counters copied to their
//                            host mirror
// Every value is a gather, a maximum or an exact power-of-two scaling followed by the same roundings: bit-identical to the stage
// kernels (tests/test_hip_parity.py::test_train_glue_is_bit_identical runs both).
#include "nerf_internal.h"

namespace nerf {

typedef float f32x4r __attribute__((ext_vector_type(4)));
typedef unsigned u32x4r __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2r __attribute__((ext_vector_type(2)));
typedef float f32x2r __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(1024) void refresh_gather_kernel(const RefreshBatch b) {
    __shared__ float red[16];
    int blk = blockIdx.x;
    for (int si = 0; si < b.n_streams; ++si) {
        const RefreshStream& st = b.st[si];
        if (blk < st.n_chunks) {
            // one chunk: stream[i] = table[i] >= 0 ? params[table[i]] : 0 (gather_kernel), and its largest |value| (chunk_absmax_kernel)
            const int* t = st.table + (size_t)blk * kChunkFloats;
            float* o = st.stream + (size_t)blk * kChunkFloats;
            float m = 0.0f;
            for (int i = threadIdx.x; i < kChunkFloats; i += 1024) {
                const int ti = t[i];
                const float v = ti >= 0 ? st.params[ti] : 0.0f;
                o[i] = v;
                m = fmaxf(m, fabsf(v));
            }
            for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
            __syncthreads();
            if (threadIdx.x == 0) {
                float mm = red[0];
                for (int w = 1; w < 16; ++w) mm = fmaxf(mm, red[w]);
                st.chunk_max[blk] = mm;
            }
            return;
        }
        blk -= st.n_chunks;
    }
    for (int bi = 0; bi < b.n_bias; ++bi) {
        const RefreshBias& bs = b.bias[bi];
        const int n_blocks = (bs.n + 1023) / 1024;
        if (blk < n_blocks) {
            const int i = blk * 1024 + threadIdx.x;
            if (i < bs.n) {
                const int ti = bs.table[i];
                bs.out[i] = ti >= 0 ? bs.params[ti] : 0.0f;
            }
            return;
        }
        blk -= n_blocks;
    }
    // the last block: the gain tables start from zero (the forward gains are integer maxima of bit patterns)
    for (int gi = 0; gi < b.n_gain; ++gi)
        for (int i = threadIdx.x; i < 2 * b.gain[gi].n; i += 1024) b.gain_out[gi][i] = 0.0f;
}

__global__ __launch_bounds__(1024) void refresh_convert_kernel(const RefreshBatch b) {
    __shared__ float part[4][256];
    __shared__ float red[2][16];
    int blk = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int si = 0; si < b.n_streams; ++si) {
        const RefreshStream& st = b.st[si];
        if (blk < st.n_chunks) {
            // convert_stream_h2_kernel for this chunk: the layer's scale from its chunks' maxima, then 1024 work items
            const int chunk = blk, layer = st.chunk_layer[chunk];
            float m = 0.0f;
            bool first = true;
            for (int i = 0; i < st.n_chunks; ++i)
                if (st.chunk_layer[i] == layer) {
                    m = fmaxf(m, st.chunk_max[i]);
                    if (i < chunk) first = false;
                }
            int e = (m > 0.0f && m < __builtin_inff()) ? 13 - __builtin_amdgcn_frexp_expf(m) : 0;
            e = e < -60 ? -60 : (e > 60 ? 60 : e);
            const float sc = __builtin_ldexpf(1.0f, e);
            if (first && threadIdx.x == 0) st.descale[layer] = __builtin_ldexpf(1.0f, -e);
            const float* src = st.stream + (size_t)chunk * kChunkFloats;
            uint32_t* dst = st.out_h2 + (size_t)chunk * kChunkFloats;
            // the kernels' weight ring runs three chunks ahead across tile boundaries: a copy of the stream's head follows its end
            uint32_t* dst2 = chunk < kStreamTailChunks ? st.out_h2 + (size_t)(st.n_chunks + chunk) * kChunkFloats : nullptr;
            const int w = threadIdx.x;      // (unit u, k-slice s, lane): 8 x 2 x 64
            const int l = w & 63, s = (w >> 6) & 1, u = w >> 7;
            const f32x4r a = *(const f32x4r*)(src + ((4 * u + 2 * s) * 64 + l) * 4);
            const f32x4r c = *(const f32x4r*)(src + ((4 * u + 2 * s + 1) * 64 + l) * 4);
            const float v[8] = {a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
            u32x4r hi, lo;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float x0 = v[2 * q] * sc, x1 = v[2 * q + 1] * sc;
                const f32x2r xx = {x0, x1};
                const h16x2r p = __builtin_convertvector(xx, h16x2r);
                const f32x2r rr = {x0 - (float)p[0], x1 - (float)p[1]};
                const h16x2r r = __builtin_convertvector(rr, h16x2r);
                hi[q] = __builtin_bit_cast(unsigned, p);
                lo[q] = __builtin_bit_cast(unsigned, r);
            }
            *(u32x4r*)(dst + ((4 * u + 2 * s) * 64 + l) * 4) = hi;
            *(u32x4r*)(dst + ((4 * u + 2 * s + 1) * 64 + l) * 4) = lo;
            if (dst2) {
                *(u32x4r*)(dst2 + ((4 * u + 2 * s) * 64 + l) * 4) = hi;
                *(u32x4r*)(dst2 + ((4 * u + 2 * s + 1) * 64 + l) * 4) = lo;
            }
            return;
        }
        blk -= st.n_chunks;
    }
    for (int gi = 0; gi < b.n_gain; ++gi) {
        // layer_gain_kernel: block = (layer, group of 16 rows), a wavefront per row
        const GainRefs& refs = b.gain[gi];
        int max_out = 1;
        for (int l = 0; l < refs.n; ++l) max_out = refs.out[l] > max_out ? refs.out[l] : max_out;
        const int groups = (max_out + 15) / 16, n_blocks = refs.n * groups;
        if (blk < n_blocks) {
            const int l = blk / groups, row = (blk % groups) * 16 + wave, n_in = refs.in[l];
            float g = 0.0f, bm = 0.0f;
            if (row < refs.out[l]) {
                const float* w = b.gain_params[gi] + refs.w_off[l] + (size_t)row * n_in;
                float s = 0.0f;
                for (int k = lane; k < n_in; k += 64) s += fabsf(w[k]);
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                g = s;
                bm = fabsf(b.gain_params[gi][refs.b_off[l] + row]);
            }
            if (lane == 0) {
                red[0][wave] = g;
                red[1][wave] = bm;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                float gm = 0.0f, bb = 0.0f;
                for (int w = 0; w < 16; ++w) {
                    gm = fmaxf(gm, red[0][w]);
                    bb = fmaxf(bb, red[1][w]);
                }
                atomicMax((int*)&b.gain_out[gi][2 * l], __float_as_int(gm));
                atomicMax((int*)&b.gain_out[gi][2 * l + 1], __float_as_int(bb));
            }
            return;
        }
        blk -= n_blocks;
    }
    for (int gi = 0; gi < b.n_bgain; ++gi) {
        // layer_gain_bwd_kernel: block = backward layer, thread = (column r, row quarter q)
        const BwdGainRefs& refs = b.bgain[gi];
        if (blk < refs.n) {
            const int l = blk, r = threadIdx.x & 255, q = threadIdx.x >> 8;
            const float* params = b.bgain_params[gi];
            const float* w = params + refs.w_off[l] + refs.col0[l] + r;
            const int n_rows = refs.rows[l], per = (n_rows + 3) / 4;
            float sum = 0.0f;
            for (int c0 = q * per; c0 < (q + 1) * per; c0 += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int c = c0 + u;
                    v[u] = w[(size_t)(c < n_rows ? c : n_rows - 1) * refs.ld[l]];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) sum += (c0 + u < (q + 1) * per && c0 + u < n_rows) ? fabsf(v[u]) : 0.0f;
            }
            part[q][r] = sum;
            __syncthreads();
            if (threadIdx.x < 256) {
                sum = part[0][r] + part[1][r] + part[2][r] + part[3][r];
                float am = (l == 1 && refs.alpha_off != 0xffffffffu) ? fabsf(params[refs.alpha_off + r]) : 0.0f;
                for (int o = 32; o > 0; o >>= 1) {
                    sum = fmaxf(sum, __shfl_xor(sum, o));
                    am = fmaxf(am, __shfl_xor(am, o));
                }
                if ((threadIdx.x & 63) == 0) {
                    red[0][threadIdx.x >> 6] = sum;
                    red[1][threadIdx.x >> 6] = am;
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                b.bgain_out[gi][2 * l] = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
                b.bgain_out[gi][2 * l + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
            }
            return;
        }
        blk -= refs.n;
    }
    // the last block: the precision guard's counters follow the step to their pinned host mirror (nerf_ctx::h_loose)
    if (b.mirror_dst && threadIdx.x < kLooseWords) {
        b.mirror_dst[threadIdx.x] = __builtin_nontemporal_load(b.mirror_src + threadIdx.x);
        __threadfence_system();
    }
}

hipError_t launch_refresh(const RefreshBatch& b, hipStream_t s) {
    if (b.n_streams < 0 || b.n_streams > 4 || b.n_bias < 0 || b.n_bias > 2 || b.n_gain < 0 || b.n_gain > 2 || b.n_bgain < 0 ||
        b.n_bgain > 2)
        return hipErrorInvalidValue;
    int chunks = 0, bias_blocks = 0, gain_blocks = 0, bgain_blocks = 0;
    for (int i = 0; i < b.n_streams; ++i) {
        if (b.st[i].n_chunks < kStreamTailChunks) return hipErrorInvalidValue;
        chunks += b.st[i].n_chunks;
    }
    for (int i = 0; i < b.n_bias; ++i) bias_blocks += (b.bias[i].n + 1023) / 1024;
    for (int i = 0; i < b.n_gain; ++i) {
        int max_out = 1;
        for (int l = 0; l < b.gain[i].n; ++l) max_out = b.gain[i].out[l] > max_out ? b.gain[i].out[l] : max_out;
        gain_blocks += b.gain[i].n * ((max_out + 15) / 16);
    }
    for (int i = 0; i < b.n_bgain; ++i) bgain_blocks += b.bgain[i].n;
    hipLaunchKernelGGL(refresh_gather_kernel, dim3((unsigned)(chunks + bias_blocks + 1)), dim3(1024), 0, s, b);
    hipLaunchKernelGGL(refresh_convert_kernel, dim3((unsigned)(chunks + gain_blocks + bgain_blocks + 1)), dim3(1024), 0, s, b);
    return hipGetLastError();
}

// ---- the view fold (PackedNet::d_stream_fold) -------------------------------------------------------------------------
// W_vf = W_v[:, :W] W_f and b_vf = W_v[:, :W] b_f + b_v from the row-equalised parameters, every entry accumulated in fp64 in
// index order and rounded once to fp32. Equalisation scales unit j of feature_linear by 2^e_j and column j of the view layer
// by 2^-e_j, so the product of the equalised matrices IS the equalised fold. 8.4 MFLOP per network: a workgroup per view
// unit, a thread per trunk unit. A workgroup also looks at every entry it reads or writes (its row of the view layer, the
// rows r, r + n_view, ... of feature_linear): one that is not finite sets word[1].
__global__ __launch_bounds__(256) void view_fold_kernel(const float* params, float* tail, const ViewFoldRefs refs, unsigned* word) {
    __shared__ float wv[kWidth];
    __shared__ double part[kWidth];
    const int r = blockIdx.x, c = threadIdx.x, W = refs.W, ld = refs.W + refs.n_dir;
    const float* row = params + refs.wv_off + (size_t)r * ld;
    const float inf = __builtin_inff();
    bool bad = false;
    for (int j = c; j < ld; j += 256) {
        const float v = row[j];
        if (j < W) wv[j] = v;
        bad = bad || !(fabsf(v) < inf);
    }
    __syncthreads();
    if (c < W) {
        double acc = 0.0;
        for (int j = 0; j < W; ++j) acc = fma((double)wv[j], (double)params[refs.wf_off + (size_t)j * W + c], acc);
        const float o = (float)acc;
        tail[(size_t)r * W + c] = o;
        bad = bad || !(fabsf(o) < inf);
        for (int j = r; j < W; j += refs.n_view) bad = bad || !(fabsf(params[refs.wf_off + (size_t)j * W + c]) < inf);
        const float bf = params[refs.bf_off + c];
        bad = bad || !(fabsf(bf) < inf);
        part[c] = (double)wv[c] * (double)bf;
    }
    __syncthreads();
    if (c == 0) {
        const float bv = params[refs.bv_off + r];
        double acc = 0.0;
        for (int j = 0; j < W; ++j) acc += part[j];
        const float o = (float)(acc + (double)bv);
        tail[(size_t)refs.n_view * W + r] = o;
        bad = bad || !(fabsf(o) < inf) || !(fabsf(bv) < inf);
    }
    if (bad) atomicOr(&word[1], 1u);
}

// Whether the fp16-pair kernel may use the fold: word[0] = 1 only if
//  * every entry of W_f, b_f, W_v, b_v, W_vf, b_vf is finite (word[1], above);
//  * feature_linear cannot overflow on any trunk output the kernel would accept: with its gain pair (largest row sum of |W_f|,
//    largest |b_f|) gain * m + bmax is finite for every m <= kFoldMaxTrunk = 2^64. The reference turns an overflowing feature
//    vector into NaN colours, which the folded kernel, never forming the vector, cannot see: a network that can overflow
//    below 2^64 keeps the unfolded path, and for the others the kernel counts a point whose trunk output is large enough
//    to make the bound infinite as a loose-bound event. 2^64 is beyond any activation a trained network
//    produces (|h| of the lego networks stays below 2^6) and leaves feature_linear 2^63 of headroom for its gain;
//  * the largest |W_vf| and the largest |W_v[:, W:]| - they share the view layer's scale in the stream - are within 2^8 of
//    each other: the larger maps to [2^12, 2^13), so the smaller block's largest entry sits at 2^4 or above and its entries
//    down to 2^-6 of that keep whole low halves (normal fp16 from 2^-2 up: Pending in mlp_kernel_h2.hip); below that the
//    absolute error 2^-25 is 2^-29 of the block's largest entry, under the fp32 rounding of the terms that dominate the sum.
//    The unfolded layer pairs W_v[:, :W] with the same columns and is not checked: it is what the kernel has always run. A
//    block of zeros (max 0) loses nothing.
constexpr float kFoldMaxTrunk = 18446744073709551616.0f;      // 2^64
__global__ void view_fold_eligible_kernel(const float* gain, int D, const float* chunk_max, int first_view, unsigned* word) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float inf = __builtin_inff();
    bool ok = word[1] == 0u;
    ok = ok && fmaf(gain[2 * D], kFoldMaxTrunk, gain[2 * D + 1]) < inf;
    float m_vf = 0.0f;
    for (int k = 0; k < 4; ++k) m_vf = fmaxf(m_vf, chunk_max[first_view + k]);
    const float m_d = chunk_max[first_view + 5];
    if (m_vf > 0.0f && m_d > 0.0f) ok = ok && m_vf <= m_d * 256.0f && m_d <= m_vf * 256.0f;
    word[0] = ok ? 1u : 0u;
}

// ---- the per-ray view bias (MlpLaunch::ray_bias) ------------------------------------------------------------------------
// In ray mode with a multiple of 32 samples per ray a wavefront's 32 points share one ray, so the view layer's gamma(dir) term
// is the same for all of them: u = b_vf + W_v[:, W:] gamma(dir) is formed here once per ray, from the equalised parameters and
// their fold tail, and nerf_mlp_h2_fold_ray_kernel reads it where the folded kernel reads b_vf and runs the gamma(dir) chunk.
// gamma(dir) is the encoder's (encode_point, mlp_inputs.h: the accurate sincosf of d * 2^k, d * 2^k exact); every entry is
// accumulated in fp64 from b_vf over the encoding columns in index order and rounded once to fp32, so a ray's row depends on
// nothing but the ray and the weights. A thread owns one entry of the row ([tile(4)][h(2)][16]: the view layer's bias-block
// order) and keeps its 27 weights in registers; a workgroup walks its rays eight at a time, their encodings shared through LDS.
constexpr int kRayBiasBatch = 8, kRayBiasPerBlock = 64;
__global__ __launch_bounds__(kRayBiasEntries) void ray_view_bias_kernel(const float* params, const ViewFoldRefs refs, const float* rays,
                                                                    int ray_ld, int64_t n_rays, float* table) {
    __shared__ float g[kRayBiasBatch][32];      // gamma(dir) by encoding column (0 beyond n_dir); [27]: max(|d|, 1)
    const int i = threadIdx.x;
    const int feat = 32 * (i >> 5) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * ((i >> 4) & 1);      // acc_feature (pack_weights.cpp)
    const int ld = refs.W + refs.n_dir;
    const bool unit = feat < refs.n_view;      // (a narrower network's missing units: zero, as in its bias tiles)
    float w[27];
#pragma unroll
    for (int c = 0; c < 27; ++c) w[c] = (unit && c < refs.n_dir) ? params[refs.wv_off + (size_t)feat * ld + refs.W + c] : 0.0f;
    const float b = unit ? params[refs.tail_off + (size_t)refs.n_view * refs.W + feat] : 0.0f;
    for (int q = i; q < kRayBiasBatch * 32; q += kRayBiasEntries) g[q >> 5][q & 31] = 0.0f;
    const int64_t first = (int64_t)blockIdx.x * kRayBiasPerBlock;
    const int64_t end = first + kRayBiasPerBlock < n_rays ? first + kRayBiasPerBlock : n_rays;
    for (int64_t base = first; base < end; base += kRayBiasBatch) {
        __syncthreads();      // the batch before has been read (first round: the zeros are in place)
        if (i < kRayBiasBatch * 12) {
            const int r = i / 12, k = (i % 12) / 3, c = i % 3;
            const int64_t ray = base + r < end ? base + r : end - 1;
            const float* d = rays + ray * ray_ld + ray_ld - 3;
            if (3 + 6 * k + c < refs.n_dir) {
                float sn, cs;
                sincosf(d[c] * (float)(1 << k), &sn, &cs);
                g[r][3 + 6 * k + c] = sn;
                g[r][3 + 6 * k + 3 + c] = cs;
            }
            if (k == 0) g[r][c] = d[c];
            // the bound load_inputs gives for |gamma(dir)| (v_max_f32 passes over a NaN component, there as here)
            if (i % 12 == 0) g[r][27] = fmaxf(fmaxf(fabsf(d[0]), fabsf(d[1])), fmaxf(fabsf(d[2]), 1.0f));
        }
        __syncthreads();
        for (int r = 0; r < kRayBiasBatch && base + r < end; ++r) {
            double acc = (double)b;
#pragma unroll
            for (int c = 0; c < 27; ++c) acc = fma((double)w[c], (double)g[r][c], acc);
            float* row = table + (base + r) * kRayBiasRow;
            row[i] = (float)acc;
            if (i < kRayBiasRow - kRayBiasEntries) row[kRayBiasMax + i] = i == 0 ? g[r][27] : 0.0f;
        }
    }
}

hipError_t launch_ray_view_bias(const float* params_eq, const ViewFoldRefs& r, const float* rays, int ray_ld, int64_t n_rays,
                                float* table, hipStream_t s) {
    if (n_rays <= 0) return hipSuccess;
    if (!params_eq || !rays || !table || ray_ld < 11 || r.n_dir < 3 || r.n_dir > 27 || r.n_view < 1 || r.n_view > kRayBiasEntries)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ray_view_bias_kernel, dim3((unsigned)((n_rays + kRayBiasPerBlock - 1) / kRayBiasPerBlock)), dim3(kRayBiasEntries),
                       0, s, params_eq, r, rays, ray_ld, n_rays, table);
    return hipGetLastError();
}

hipError_t launch_view_fold(const float* params_eq, float* tail, const ViewFoldRefs& r, unsigned* word, hipStream_t s) {
    if (!params_eq || !tail || !word || r.W < 2 || r.W > kWidth || r.n_view < 1 || r.n_dir < 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(word, 0, 2 * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(view_fold_kernel, dim3((unsigned)r.n_view), dim3(256), 0, s, params_eq, tail, r, word);
    return hipGetLastError();
}

hipError_t launch_view_fold_eligible(const float* gain, int D, const float* chunk_max, int first_view, unsigned* word,
                                     hipStream_t s) {
    hipLaunchKernelGGL(view_fold_eligible_kernel, dim3(1), dim3(64), 0, s, gain, D, chunk_max, first_view, word);
    return hipGetLastError();
}

}  // namespace nerf
