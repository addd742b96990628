// rs_cnn_sized_bwd.inc -- the body of the tiled trunk's backward kernels (rs_cnn_sized.hip), included once by rs_sized_trunk_bwd (OCC =
// false) and once by rs_sized_trunk_bwd_occ (OCC = true, flags).  Text, not an inlined function: moved into a function, hipcc schedules
// the dense kernel differently, and that kernel's code is to stay as it is.  In scope at the include: CIN, OCC, in, w2, da2, relu_mask,
// p1g, amax, flags, slab.
    __shared__ __align__(16) float smem[DP * BWS * BWS + C1 * HC + C2 * HC + C1 * NT + 2 * NT];
    float* xs = smem;                         // input window [plane][34][34]
    float* ps = xs + DP * BWS * BWS;          // P1 with halo [ci][18][18]
    float* dz = ps + C1 * HC;                 // dZ2 = ReLU-gated da2 with halo [co][18][18]
    float* gb = dz + C2 * HC;                 // dL/d(P1) gated by P1 > 0, the tile's cells [ci][256]
    uint8_t* am = reinterpret_cast<uint8_t*>(gb + C1 * NT);     // arg-max codes of the tile's cells [256][8]
    constexpr int K1 = CIN * 9, CH0 = (CIN == 6) ? 2 : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = in.P, PP = P * P;
    const int ly = tid / TS, lx = tid - ly * TS;
    // dW2 / db2: thread = (output channel co2, input channel ci2, half of the tile's rows) -> 9 taps + db2;
    // dW1 / db1: thread = (output channel co1, plane pair, tile row ly) -> 2 x 9 taps + db1
    const int co2 = tid & 15, ci2 = (tid >> 4) & 7, half2 = tid >> 7;
    const int co1 = tid & 7, half = (tid >> 3) & 1;
    float aw2[10], aw1[19], gst = 0.0f;
#pragma unroll
    for (int k = 0; k < 10; ++k) aw2[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 19; ++k) aw1[k] = 0.0f;
    // OCC, the empty units: thread = (output channel co2, tile row tid >> 4) -> es[ky][kx] = its row's part of S, er[ky][kx] of R
    // (the sums of dZ2 that dW2 / db2 and db1 reduce to where P1 is the per-channel constant c1; see the fold behind the unit loop);
    // ecell: a pooled cell of the first empty unit, whose p1 is c1
    float es[9], er[9];
    long long ecell = -1;
#pragma unroll
    for (int k = 0; k < 9; ++k) { es[k] = 0.0f; er[k] = 0.0f; }
    const int nt2 = in.ntile * in.ntile;
    const long long units = in.S * nt2;
    uint8_t ahead = OCC && blockIdx.x < units ? flags[blockIdx.x] : 1;     // a unit's flag is read one unit ahead: no unit starts with a wait for it
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const uint8_t flag = ahead;
        if (OCC && u + gridDim.x < units) ahead = flags[u + gridDim.x];
        const long long s = u / nt2;
        const int tile = (int)(u - s * nt2), ty0 = (tile / in.ntile) * TS, tx0 = (tile % in.ntile) * TS;
        int loc, pc;
        owner_cells(in, s, loc, pc);
        if (OCC && unit_is_empty(in, flag, ty0, tx0, loc, pc)) {
            // dZ2 with its halo is all an empty unit reads: no input window, no p1, no arg-max codes
            // Both trips' loads are issued before the first is used, and da2 is read whatever the mask says (the gate is a select
            // behind the load): one memory latency per unit in place of four
            float gv[2][C2];
            uint32_t live[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int h = tid + t * NT, hy = h / HS, hx = h - hy * HS, gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
                const bool in_map = h < HC && gy >= 0 && gy < P && gx >= 0 && gx < P;
                const size_t cell = (size_t)s * PP + (in_map ? gy * P + gx : 0);
                live[t] = in_map ? relu_mask[cell] : 0u;
                const float* g = da2 + (size_t)s * C2 * PP + (in_map ? gy * P + gx : 0);
#pragma unroll
                for (int co = 0; co < C2; ++co) gv[t][co] = in_map ? g[(size_t)co * PP] : 0.0f;
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int h = tid + t * NT;
                if (h < HC) {
#pragma unroll
                    for (int co = 0; co < C2; ++co) dz[co * HC + h] = ((live[t] >> co) & 1u) ? gv[t][co] : 0.0f;
                }
            }
            __syncthreads();
            {
                const int row = tid >> 4, gy = ty0 + row, nx = min(TS, P - tx0);
                const float* hrow = dz + co2 * HC + row * HS;          // halo rows row .. row + 2 = the pixel rows gy - 1 .. gy + 1
                float h[3][HS];
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int x = 0; x < HS; ++x) h[j][x] = hrow[j * HS + x];
                // S[ky][kx]: the row's own pixels (y, x) whose neighbour (y + ky - 1, x + kx - 1) is inside the map (dZ2 is 0 outside it)
                float t[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int x = 0; x < TS; ++x) {
                    const float v = h[1][x + 1];
                    t[0] += tx0 + x >= 1 ? v : 0.0f;
                    t[1] += v;
                    t[2] += tx0 + x + 1 < P ? v : 0.0f;
                }
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    es[kx] += gy >= 1 ? t[kx] : 0.0f;
                    es[3 + kx] += t[kx];
                    es[6 + kx] += gy + 1 < P ? t[kx] : 0.0f;
                }
                // R[ky][kx]: dZ2 at (cy - ky + 1, cx - kx + 1) over the row's own cells (cy, cx) inside the map
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        float r = 0.0f;
#pragma unroll
                        for (int x = 0; x < TS; ++x) r += x < nx ? h[2 - ky][x + 2 - kx] : 0.0f;
                        er[ky * 3 + kx] += gy < P ? r : 0.0f;
                    }
            }
            if (ecell < 0) ecell = s * PP + (long long)ty0 * P + tx0;
            __syncthreads();
            continue;
        }
        cmem_t w2c = as_cmem(w2);                 // per iteration, as in the forward kernel
        asm volatile("" : "+s"(w2c));
        stage_window<BWS>(in, s, 2 * ty0 - 1, 2 * tx0 - 1, xs);
#pragma unroll 1
        for (int h = tid; h < HC; h += NT) {
            const int hy = h / HS, hx = h - hy * HS, gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
            const bool in_map = gy >= 0 && gy < P && gx >= 0 && gx < P;
            const size_t cell = (size_t)s * PP + (in_map ? gy * P + gx : 0);
            float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), pb = pa;
            uint32_t live = 0u;
            if (in_map) {
                pa = reinterpret_cast<const float4*>(p1g + cell * C1)[0];
                pb = reinterpret_cast<const float4*>(p1g + cell * C1)[1];
                live = relu_mask[cell];
            }
            ps[0 * HC + h] = pa.x; ps[1 * HC + h] = pa.y; ps[2 * HC + h] = pa.z; ps[3 * HC + h] = pa.w;
            ps[4 * HC + h] = pb.x; ps[5 * HC + h] = pb.y; ps[6 * HC + h] = pb.z; ps[7 * HC + h] = pb.w;
            const float* g = da2 + (size_t)s * C2 * PP + (in_map ? gy * P + gx : 0);
#pragma unroll
            for (int co = 0; co < C2; ++co) dz[co * HC + h] = ((live >> co) & 1u) ? g[(size_t)co * PP] : 0.0f;
        }
        {
            const int gy = ty0 + ly, gx = tx0 + lx;
            uint2 code = make_uint2(0u, 0u);
            if (gy < P && gx < P) code = *reinterpret_cast<const uint2*>(amax + ((size_t)s * PP + gy * P + gx) * C1);
            *reinterpret_cast<uint2*>(am + tid * C1) = code;
        }
        __syncthreads();
        // ---- dW2[co][ci][ky][kx] += sum_px dZ2[co][px] P1[ci][px + (ky - 1, kx - 1)], db2[co] += sum_px dZ2[co][px]: eight rows of 16
        // pixels; a P1 row of 18 values serves the three kx taps of all 16 pixels of a row
#pragma unroll 1
        for (int yy = 0; yy < TS / 2; ++yy) {
            const int y = half2 * (TS / 2) + yy;
            float dzr[TS];
#pragma unroll
            for (int x = 0; x < TS; ++x) { dzr[x] = dz[co2 * HC + (y + 1) * HS + x + 1]; aw2[9] += dzr[x]; }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                float r[HS];
#pragma unroll
                for (int x = 0; x < HS; ++x) r[x] = ps[ci2 * HC + (y + ky) * HS + x];
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int x = 0; x < TS; ++x) aw2[ky * 3 + kx] = __builtin_fmaf(dzr[x], r[x + kx], aw2[ky * 3 + kx]);
            }
        }
        // ---- dP1[ci][cell] = sum_{co,ky,kx} w2[co][ci][ky][kx] dZ2[co][cell - (ky - 1, kx - 1)], gated by P1 > 0 (cells outside the map have
        // P1 = 0 in ps: no gradient)
        {
            float g[C1];
#pragma unroll
            for (int ci = 0; ci < C1; ++ci) g[ci] = 0.0f;
            const float* dq = dz + (ly + 2) * HS + lx + 2;
#pragma unroll 1
            for (int q = 0; q < C2 * 3; ++q) {               // rolled over (co, ky): 24 weights per trip
                const int co = q / 3, ky = q - co * 3;
                const cmem_t wq = w2c + co * 72 + ky * 3;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = dq[co * HC - ky * HS - kx];
#pragma unroll
                    for (int ci = 0; ci < C1; ++ci) g[ci] = __builtin_fmaf(wq[ci * 9 + kx], v, g[ci]);
                }
            }
#pragma unroll
            for (int ci = 0; ci < C1; ++ci) gb[ci * NT + tid] = ps[ci * HC + (ly + 1) * HS + lx + 1] > 0.0f ? g[ci] : 0.0f;
        }
        __syncthreads();
        // ---- dW1[co1][plane][ky][kx] += g[co1][cell] x[plane] at the cell's arg-max pixel + (ky - 1, kx - 1); db1[co1] += g
        {
#pragma unroll 1
            for (int x = 0; x < TS; ++x) {
                const int cell = ly * TS + x;
                const float gv = gb[co1 * NT + cell];
                const int code = am[cell * C1 + co1];
                const float* base = xs + (2 * half) * BWS * BWS + (2 * ly + (code >> 1)) * BWS + 2 * x + (code & 1);
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int kk = 0; kk < 9; ++kk) aw1[j * 9 + kk] = __builtin_fmaf(gv, base[j * BWS * BWS + (kk / 3) * BWS + kk % 3], aw1[j * 9 + kk]);
                aw1[18] += gv;
            }
        }
        if (CIN == 6 && tid < 2 * C1 * 9) {
            // the one-hot channels: input (r, c) meets tap (ky, kx) at conv pixel (r - ky + 1, c - kx + 1), which carries gradient iff it
            // is its pool window's arg-max for channel co; the tile that owns the pooled cell adds it
            const int which = tid / (C1 * 9), co = (tid % (C1 * 9)) / 9, kk = tid % 9;
            const int at = which ? loc : pc;
            if (at >= 0) {
                const int r = at / in.M, c = at - r * in.M;
                const int y = r - kk / 3 + 1, x = c - kk % 3 + 1;
                if (y >= 0 && y < 2 * P && x >= 0 && x < 2 * P) {
                    const int cy = (y >> 1) - ty0, cx = (x >> 1) - tx0;
                    if (cy >= 0 && cy < TS && cx >= 0 && cx < TS && am[(cy * TS + cx) * C1 + co] == (uint8_t)((y & 1) * 2 + (x & 1)))
                        gst += gb[co * NT + cy * TS + cx];
                }
            }
        }
        __syncthreads();
    }
    // ---- workgroup reduction in a fixed order.  dW1: the four tile rows of a wave by lane swaps (lanes l, l ^ 16, l ^ 32), then the
    // four waves; dW2: the two row halves
#pragma unroll
    for (int k = 0; k < 19; ++k) { aw1[k] += __shfl_xor(aw1[k], 16); aw1[k] += __shfl_xor(aw1[k], 32); }
    float* red2 = smem;                        // [2 halves][8 ci][16 co][10]
    float* red1 = red2 + NT * 10;              // [4 waves][16 (co1, half)][19]
    float* gred = red1 + 4 * 16 * 19;          // [2][8][9]
#pragma unroll
    for (int k = 0; k < 10; ++k) red2[tid * 10 + k] = aw2[k];
    if (lane < 16) {
#pragma unroll
        for (int k = 0; k < 19; ++k) red1[(wave * 16 + lane) * 19 + k] = aw1[k];
    }
    if (tid < 2 * C1 * 9) gred[tid] = gst;
    // OCC: the empty units' sums over the 16 tile rows in a fixed order -> tot [16 co][S 9 | R 9]; c1 and w2 are folded in below, once
    float* erow = gred + 2 * C1 * 9;           // [16 rows][16 co][18]
    float* tot = erow + NT * 18;               // [16 co][18]
    if (OCC) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { erow[tid * 18 + k] = es[k]; erow[tid * 18 + 9 + k] = er[k]; }
    }
    auto c1 = [&](int ci) { return ecell >= 0 ? p1g[(size_t)ecell * C1 + ci] : 0.0f; };     // max(0 + b1[ci], 0), as the forward stored it
    __syncthreads();
    if (OCC) {
        for (int e = tid; e < C2 * 18; e += NT) {
            const int co = e / 18, k = e - co * 18;
            float sum = 0.0f;
#pragma unroll
            for (int r = 0; r < TS; ++r) sum += erow[((r * C2) + co) * 18 + k];
            tot[e] = sum;
        }
        __syncthreads();
    }
    constexpr int ROW = C1 * K1 + C1 + C2 * 72 + C2;
    float* out = slab + (size_t)blockIdx.x * ROW;
    for (int e = tid; e < ROW; e += NT) {
        float sum = 0.0f;
        if (e < C1 * K1) {
            const int o1 = e / K1, k = e - o1 * K1, i0 = k / 9, kk = k - i0 * 9;     // i0: the logical input channel
            if (i0 < CH0) { out[e] = gred[(i0 * C1 + o1) * 9 + kk]; continue; }   // prediction (0) / location (1): the stamp gathers
            const int d = i0 - CH0, combo = o1 + 8 * (d >> 1), slot = (d & 1) * 9 + kk;
            if (CIN == 6 && d == 0) sum = -gred[(C1 + o1) * 9 + kk];                 // others = combined - location
#pragma unroll
            for (int w = 0; w < 4; ++w) sum += red1[(w * 16 + combo) * 19 + slot];
        } else if (e < C1 * K1 + C1) {
            const int o1 = e - C1 * K1;
#pragma unroll
            for (int w = 0; w < 4; ++w) sum += red1[(w * 16 + o1) * 19 + 18];
            if (OCC) {
                // the empty units' cells: dP1[o1] = sum_{co, tap} w2[co][o1][tap] R[co][tap], gated by their P1 = c1 > 0
                float g = 0.0f;
                for (int q = 0; q < C2 * 9; ++q) g = __builtin_fmaf(w2[(q / 9) * 72 + o1 * 9 + q % 9], tot[(q / 9) * 18 + 9 + q % 9], g);
                sum += c1(o1) > 0.0f ? g : 0.0f;
            }
        } else if (e < C1 * K1 + C1 + C2 * 72) {
            const int q = e - (C1 * K1 + C1), co = q / 72, k = q - co * 72, ci = k / 9, kk = k - ci * 9;
            sum = red2[(ci * 16 + co) * 10 + kk] + red2[(NT / 2 + ci * 16 + co) * 10 + kk];
            if (OCC) {
                // the empty units' pixels see P1 = c1[ci] wherever the tap's neighbour is inside the map
                sum = __builtin_fmaf(c1(ci), tot[co * 18 + kk], sum);
            }
        } else {
            const int co = e - (C1 * K1 + C1 + C2 * 72);
            sum = red2[co * 10 + 9] + red2[(NT / 2 + co) * 10 + 9];
            if (OCC) sum += tot[co * 18 + 4];          // S of the centre tap = the sum over the units' pixels
        }
        out[e] = sum;
    }
