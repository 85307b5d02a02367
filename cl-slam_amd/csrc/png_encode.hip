// PNG files written on the device (include/clslam_hip.h "PNG encoding"): scanline filter, a deflate stream of literal-only dynamic
// (or stored) blocks, and the container with its Adler-32 and CRC-32, for n images of one size per call.
//
// LAUNCHES of clslam_png_encode, all on the caller's stream: memset(out) | filter | plan | layout | pack | finish.
//   filter  grid (h, n)     one workgroup per scanline: the five filters' scores sum(min(b, 256 - b)), reduced in LDS; the best
//                           (lowest type on ties) is formed again and written behind its type byte.
//   plan    grid (B, n)     one workgroup per block of S = kS filtered bytes: histogram (LDS atomics) of 256 literals + end-of-block,
//                           symbols ranked by (count, symbol) in parallel, the tree by the two-queue construction on thread 0 (leaves
//                           before internal nodes on ties: the optimal tree of least depth), depths by walking up in parallel, the
//                           15-bit limit by moving leaves down (only when the limit binds).  Writes the 257 code lengths, the
//                           dynamic form's bit count and the block's Adler pair (sum d, sum (len - i) d_i) mod 65521.
//   layout  grid (n)        per image: the blocks' start bits in order (a stored block pads to a byte, so the position decides
//                           between the two forms: dynamic iff it ends first), the Adler-32 from the pairs, every container byte
//                           but the IDAT CRC, the file's length.
//   pack    grid (B, n)     the block's bits, formed in LDS at the bit offset they have in the file's 32-bit words: canonical codes
//                           (bit-reversed) from the lengths, an exclusive scan of the threads' bit counts, each thread shifting its
//                           64 bytes' codes through a 64-bit register.  Then the words go out: whole words by plain coalesced stores,
//                           the first and last, which neighbours share, by atomicAdd into the zeroed file (disjoint bits: no carry, no
//                           order dependence).  The same LDS words give the block's CRC remainder (bits of neighbours are 0 there,
//                           and the remainder is linear), slicing-by-4 per thread and a tree over the threads with fixed powers.
//   finish  grid (n)        IDAT CRC = xor of the remainders, each times x^(8 * bytes between it and the CRC) mod P, + the
//                           container's own bytes + the effect of the all-ones preset.
// Bytes that share a 32-bit word with another writer are always ADDED (put_bytes / atomicAdd), never stored.
//
// CRC arithmetic is in the reflected representation zlib uses: bit 31 is x^0.  "Remainder" below is the pure one (preset 0, no final
// xor): rem(A || B) = rem(A) * x^(8 |B|) + rem(B), and crc32(M) = rem(M) ^ 0xffffffff * x^(8 |M|) ^ 0xffffffff.
#include "common.h"

namespace clslam {

constexpr int kS = CLSLAM_PNG_BLOCK;          // filtered bytes per deflate block
constexpr int kPngThreads = 256;
constexpr int kChunk = kS / kPngThreads;      // 64 bytes of a block per thread
constexpr int kSyms = 257;                    // 256 literals + end-of-block
constexpr int kLenStride = 272;               // bytes of scratch per block's code lengths
constexpr int kHeaderBits = 17 + 19 * 3 + 258 * 4;        // 1106: BFINAL BTYPE HLIT HDIST HCLEN | code-length code | 257 + 1 lengths
constexpr int kStageWords = kS / 4 + 8;       // a stored block at bit offset 31: 31 + 10 + 32 + 8 S bits
constexpr int kCrcWords = (kStageWords + kPngThreads - 1) / kPngThreads;      // words of the staged block per thread
constexpr unsigned kPoly = 0xedb88320u;
constexpr unsigned kAdlerMod = 65521u;
constexpr int kFileHead = 43;                 // signature 8, IHDR 25, IDAT length + type 8, zlib header 2: the deflate stream's offset
constexpr unsigned kStoredFlag = 0x80000000u;

static_assert(kChunk == 64 && kS % 16 == 0, "a thread's share of a block is four 16-byte loads");

__host__ __device__ constexpr unsigned gf_mul(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
    }
    return p;
}

// x^(2^k) mod P
__host__ __device__ constexpr unsigned gf_x2k(int k) {
    unsigned v = 0x40000000u;
    for (int i = 0; i < k; ++i) v = gf_mul(v, v);
    return v;
}

// x^(8 * nbytes) mod P
__host__ __device__ constexpr unsigned gf_xpow_bytes(unsigned long long nbytes) {
    unsigned r = 0x80000000u, sq = gf_x2k(3);
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1u) r = gf_mul(r, sq);
        sq = gf_mul(sq, sq);
    }
    return r;
}

// remainder of `rem` followed by one more byte
__host__ __device__ constexpr unsigned crc_byte(unsigned rem, unsigned byte) {
    rem ^= byte;
    for (int i = 0; i < 8; ++i) rem = (rem >> 1) ^ ((rem & 1u) ? kPoly : 0u);
    return rem;
}

// x^(32 * kCrcWords * 2^k): joins two runs of 2^k threads' words in the pack kernel's tree
template <int K>
struct CrcJoin {
    static constexpr unsigned value = gf_xpow_bytes((unsigned long long)4 * kCrcWords << K);
};

__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kPngThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    v = red[0];
    __syncthreads();
    return v;
}

// ---- filter ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ unsigned filter_byte(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (unsigned)(x - pred) & 255u;
}

__device__ __forceinline__ unsigned filter_score(unsigned v) { return v < 128u ? v : 256u - v; }

// grid (h, n): image (n,h,rowbytes), filtered rows of 1 + rowbytes bytes; fixed < 0: adaptive
__global__ __launch_bounds__(256) void png_filter_kernel(const unsigned char* __restrict__ image, unsigned char* __restrict__ filtered,
                                                         long long filtered_stride, int h, int rowbytes, int bpp, int fixed) {
    __shared__ unsigned red[kPngThreads];
    __shared__ unsigned best_s;
    const int tid = threadIdx.x, y = blockIdx.x;
    const unsigned char* row = image + ((size_t)blockIdx.y * h + y) * rowbytes;
    const unsigned char* up = row - rowbytes;                       // read for y > 0 only
    unsigned char* dst = filtered + (size_t)blockIdx.y * filtered_stride + (size_t)y * (rowbytes + 1);
    int type = fixed;
    if (fixed < 0) {
        unsigned s[5] = {0, 0, 0, 0, 0};
        for (int i = tid; i < rowbytes; i += kPngThreads) {
            const int x = row[i], a = i >= bpp ? row[i - bpp] : 0, b = y ? up[i] : 0, c = (y && i >= bpp) ? up[i - bpp] : 0;
#pragma unroll
            for (int t = 0; t < 5; ++t) s[t] += filter_score(filter_byte(t, x, a, b, c));
        }
        unsigned best = 0, best_v = 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const unsigned v = block_sum(s[t], red);
            if (t == 0 || v < best_v) { best = t; best_v = v; }     // strict: ties keep the lower type
        }
        if (tid == 0) best_s = best;
        __syncthreads();
        type = (int)best_s;
    }
    if (tid == 0) dst[0] = (unsigned char)type;
    for (int i = tid; i < rowbytes; i += kPngThreads) {
        const int x = row[i], a = i >= bpp ? row[i - bpp] : 0, b = y ? up[i] : 0, c = (y && i >= bpp) ? up[i - bpp] : 0;
        dst[1 + i] = (unsigned char)filter_byte(type, x, a, b, c);
    }
}

// ---- a thread's 64 bytes of a block ------------------------------------------------------------------------------------------
// p: 16-byte aligned; count in 0..64 bytes are the block's, the rest reads as 0 and is not touched in memory
__device__ __forceinline__ void load_chunk(const unsigned char* __restrict__ p, int count, unsigned (&w)[16]) {
    if (count == kChunk) {
        const int4* q = reinterpret_cast<const int4*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int4 v = q[i];
            w[4 * i] = (unsigned)v.x; w[4 * i + 1] = (unsigned)v.y; w[4 * i + 2] = (unsigned)v.z; w[4 * i + 3] = (unsigned)v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            unsigned v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) v |= (4 * i + j < count ? (unsigned)p[4 * i + j] : 0u) << (8 * j);
            w[i] = v;
        }
    }
}

__device__ __forceinline__ unsigned chunk_byte(const unsigned (&w)[16], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

// ---- plan ----------------------------------------------------------------------------------------------------------------------
// grid (B, n).  lens (n, B, kLenStride) bytes, dyn_bits / adler_a / adler_b (n, B)
__global__ __launch_bounds__(256) void png_plan_kernel(const unsigned char* __restrict__ filtered, long long filtered_stride, int F,
                                                       unsigned char* __restrict__ lens, unsigned* __restrict__ dyn_bits,
                                                       unsigned* __restrict__ adler_a, unsigned* __restrict__ adler_b) {
    __shared__ unsigned hist[kSyms + 3];
    __shared__ unsigned red[kPngThreads];
    __shared__ unsigned node_freq[2 * kSyms];
    __shared__ unsigned short parent[2 * kSyms];
    __shared__ unsigned short sorted_sym[kSyms + 3];
    __shared__ unsigned char depth[kSyms + 3];            // by rank
    __shared__ unsigned char len_of[kSyms + 3];           // by symbol
    __shared__ unsigned over_s;
    const int tid = threadIdx.x, blk = blockIdx.x, B = gridDim.x;
    const int L = min(kS, F - blk * kS);                  // >= 1
    const size_t rec = (size_t)blockIdx.y * B + blk;
    const unsigned char* src = filtered + (size_t)blockIdx.y * filtered_stride + (size_t)blk * kS + tid * kChunk;
    const int count = max(0, min(kChunk, L - tid * kChunk));

    for (int s = tid; s < kSyms + 3; s += kPngThreads) { hist[s] = s == 256 ? 1u : 0u; len_of[s] = 0; }
    if (tid == 0) over_s = 0;
    __syncthreads();
    unsigned w[16];
    load_chunk(src, count, w);
    unsigned a = 0, b = 0;
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
        if (k < count) {
            const unsigned d = chunk_byte(w, k);
            atomicAdd(&hist[d], 1u);
            a += d;
            b += (unsigned)(count - k) * d;
        }
    }
    // Adler pair of the block: sum d and sum (L - i) d_i; this thread's bytes are followed by `rest` more of the block
    const unsigned rest = (unsigned)(L - tid * kChunk - count);
    const unsigned bt = count ? (unsigned)((b + (unsigned long long)a * rest) % kAdlerMod) : 0u;
    const unsigned A = block_sum(a, red) % kAdlerMod;     // a <= 64 * 255 per thread
    const unsigned Bv = block_sum(bt, red) % kAdlerMod;
    if (tid == 0) { adler_a[rec] = A; adler_b[rec] = Bv; }

    // rank of every used symbol by (count, symbol): thread t takes symbol t, thread 0 end-of-block as well
    const unsigned n = block_sum((hist[tid] != 0u) + (tid == 0 ? 1u : 0u), red);          // >= 2: a literal and end-of-block
    for (int s = tid; s < kSyms; s += kPngThreads) {
        const unsigned f = hist[s];
        if (f) {
            unsigned r = 0;
            for (int j = 0; j < kSyms; ++j) {
                const unsigned g = hist[j];
                r += (g != 0u && (g < f || (g == f && j < s))) ? 1u : 0u;
            }
            node_freq[r] = f;
            sorted_sym[r] = (unsigned short)s;
        }
    }
    __syncthreads();
    if (tid == 0) {                                       // leaves 0..n-1 in rank order, internal nodes n..2n-2 in creation order
        unsigned i = 0, j = n, next = n;
        while (next < 2 * n - 1) {
            unsigned pick[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const bool leaf = i < n && (j >= next || node_freq[i] <= node_freq[j]);      // a leaf first on ties
                pick[q] = leaf ? i++ : j++;
            }
            node_freq[next] = node_freq[pick[0]] + node_freq[pick[1]];
            parent[pick[0]] = (unsigned short)next;
            parent[pick[1]] = (unsigned short)next;
            ++next;
        }
    }
    __syncthreads();
    for (unsigned r = tid; r < n; r += kPngThreads) {
        unsigned d = 0;
        for (unsigned v = r; v != 2 * n - 2; v = parent[v]) ++d;
        depth[r] = (unsigned char)min(d, 255u);
        if (d > 15u) over_s = 1u;
    }
    __syncthreads();
    if (over_s && tid == 0) {                             // the limit binds: clamp, then restore Kraft = 1 by moving leaves down
        unsigned count_of[16];
        for (int l = 0; l < 16; ++l) count_of[l] = 0;
        for (unsigned r = 0; r < n; ++r) count_of[min((unsigned)depth[r], 15u)]++;
        unsigned total = 0;
        for (int l = 1; l <= 15; ++l) total += count_of[l] << (15 - l);
        while (total > (1u << 15)) {                      // each round: one leaf leaves 15, a leaf at l < 15 becomes two at l + 1
            count_of[15]--;
            for (int l = 14; l > 0; --l) {
                if (count_of[l]) { count_of[l]--; count_of[l + 1] += 2; break; }
            }
            --total;
        }
        unsigned r = 0;                                   // rank 0 is the rarest symbol: the longest codes first
        for (int l = 15; l >= 1; --l) {
            for (unsigned k = 0; k < count_of[l]; ++k) depth[r++] = (unsigned char)l;
        }
    }
    __syncthreads();
    for (unsigned r = tid; r < n; r += kPngThreads) len_of[sorted_sym[r]] = depth[r];
    __syncthreads();
    unsigned bits = hist[tid] * len_of[tid] + (tid == 0 ? len_of[256] : 0u);
    bits = block_sum(bits, red);
    if (tid == 0) dyn_bits[rec] = bits + kHeaderBits;
    for (int s = tid; s < kLenStride; s += kPngThreads) lens[rec * kLenStride + s] = s < kSyms ? len_of[s] : 0;
}

// ---- layout --------------------------------------------------------------------------------------------------------------------
// bytes into zeroed words that other writers share
__device__ __forceinline__ void put_byte(unsigned* words, unsigned off, unsigned v) { atomicAdd(&words[off >> 2], v << (8 * (off & 3))); }
__device__ __forceinline__ void put_be32(unsigned* words, unsigned off, unsigned v) {
    put_byte(words, off, v >> 24); put_byte(words, off + 1, (v >> 16) & 255u); put_byte(words, off + 2, (v >> 8) & 255u);
    put_byte(words, off + 3, v & 255u);
}
__device__ __forceinline__ void put_tag(unsigned* words, unsigned off, const char* tag) {
    for (int i = 0; i < 4; ++i) put_byte(words, off + i, (unsigned char)tag[i]);
}

// grid (n).  start (n, B): the block's first bit in the deflate stream, | kStoredFlag; meta (n, 2): deflate bytes, -
__global__ __launch_bounds__(256) void png_layout_kernel(const unsigned* __restrict__ dyn_bits, const unsigned* __restrict__ adler_a,
                                                         const unsigned* __restrict__ adler_b, unsigned* __restrict__ start,
                                                         unsigned* __restrict__ meta, unsigned char* __restrict__ out,
                                                         long long out_stride, int* __restrict__ lengths, int B, int F, int h, int w,
                                                         int channels) {
    __shared__ unsigned sd[kPngThreads];
    __shared__ unsigned red[kPngThreads];
    __shared__ unsigned pos_s;
    const int tid = threadIdx.x, img = blockIdx.x;
    const size_t rec0 = (size_t)img * B;
    if (tid == 0) pos_s = 0;
    for (int c0 = 0; c0 < B; c0 += kPngThreads) {
        const int k = c0 + tid;
        __syncthreads();
        if (k < B) sd[tid] = dyn_bits[rec0 + k];
        __syncthreads();
        if (tid == 0) {
            unsigned pos = pos_s;
            const int m = min(kPngThreads, B - c0);
            for (int q = 0; q < m; ++q) {
                const unsigned L = (unsigned)min(kS, F - (c0 + q) * kS);
                const unsigned end_stored = ((pos + 3u + 7u) & ~7u) + 32u + 8u * L, end_dynamic = pos + sd[q];
                const bool stored = end_dynamic >= end_stored;
                sd[q] = pos | (stored ? kStoredFlag : 0u);
                pos = stored ? end_stored : end_dynamic;
            }
            pos_s = pos;
        }
        __syncthreads();
        if (k < B) start[rec0 + k] = sd[tid];
    }
    __syncthreads();
    const unsigned deflate_bytes = (pos_s + 7u) >> 3;

    // Adler-32 of the F filtered bytes: a = 1 + sum A_k, b = F + sum (B_k + A_k * bytes after block k)
    unsigned sa = 0, sb = 0;
    for (int k = tid; k < B; k += kPngThreads) {
        const unsigned A = adler_a[rec0 + k];
        const unsigned after = (unsigned)(F - min(F, (k + 1) * kS)) % kAdlerMod;
        sa = (sa + A) % kAdlerMod;
        sb = (sb + adler_b[rec0 + k] + (unsigned)((unsigned long long)A * after % kAdlerMod)) % kAdlerMod;
    }
    const unsigned a = (block_sum(sa, red) + 1u) % kAdlerMod;
    const unsigned b = (block_sum(sb, red) + (unsigned)F % kAdlerMod) % kAdlerMod;
    if (tid != 0) return;
    const unsigned adler = (b << 16) | a;
    unsigned* words = reinterpret_cast<unsigned*>(out + (size_t)img * out_stride);
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (int i = 0; i < 8; ++i) put_byte(words, i, sig[i]);
    put_be32(words, 8, 13u);
    const unsigned char ihdr[17] = {'I', 'H', 'D', 'R', (unsigned char)(w >> 24), (unsigned char)(w >> 16), (unsigned char)(w >> 8),
                                    (unsigned char)w, (unsigned char)(h >> 24), (unsigned char)(h >> 16), (unsigned char)(h >> 8),
                                    (unsigned char)h, 8, (unsigned char)(channels == 3 ? 2 : 0), 0, 0, 0};
    unsigned crc = 0xffffffffu;
    for (int i = 0; i < 17; ++i) { put_byte(words, 12 + i, ihdr[i]); crc = crc_byte(crc, ihdr[i]); }
    put_be32(words, 29, crc ^ 0xffffffffu);
    put_be32(words, 33, deflate_bytes + 6u);
    put_tag(words, 37, "IDAT");
    put_byte(words, 41, 0x78u);
    put_byte(words, 42, 0x01u);
    const unsigned tail = kFileHead + deflate_bytes;
    put_be32(words, tail, adler);                         // tail + 4: the IDAT CRC (finish)
    put_be32(words, tail + 8, 0u);
    put_tag(words, tail + 12, "IEND");
    put_be32(words, tail + 16, 0xae426082u);
    lengths[img] = (int)(tail + 20u);
    meta[2 * img] = deflate_bytes;
    meta[2 * img + 1] = adler;
}

// ---- pack ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_bits(unsigned* stage, unsigned pos, unsigned value, int nbits) {      // nbits <= 32
    const unsigned sh = pos & 31u;
    atomicAdd(&stage[pos >> 5], value << sh);
    if (sh && sh + (unsigned)nbits > 32u) atomicAdd(&stage[(pos >> 5) + 1], value >> (32u - sh));
}

__device__ __forceinline__ unsigned reverse_bits(unsigned v, int nbits) {
    unsigned r = 0;
    for (int i = 0; i < nbits; ++i) r |= ((v >> i) & 1u) << (nbits - 1 - i);
    return r;
}

template <int K>
__device__ __forceinline__ void crc_tree(unsigned* red, int tid) {
    if ((tid & ((2 << K) - 1)) == 0) red[tid] = gf_mul(red[tid], CrcJoin<K>::value) ^ red[tid + (1 << K)];
    __syncthreads();
    if constexpr (K < 7) crc_tree<K + 1>(red, tid);
}

// grid (B, n).  crc_rem / crc_end (n, B): the remainder of the block's bits as they lie in the file's words (everything else 0)
// and the file offset just behind the last of those words
__global__ __launch_bounds__(256) void png_pack_kernel(const unsigned char* __restrict__ filtered, long long filtered_stride, int F,
                                                       const unsigned char* __restrict__ lens, const unsigned* __restrict__ start,
                                                       unsigned char* __restrict__ out, long long out_stride,
                                                       unsigned* __restrict__ crc_rem, unsigned* __restrict__ crc_end) {
    __shared__ unsigned stage[kStageWords];
    __shared__ unsigned table[kSyms + 3];                 // reversed code | length << 16
    __shared__ unsigned char len_of[kLenStride];
    __shared__ unsigned scan[kPngThreads];
    __shared__ unsigned crc_t[4][256];
    const int tid = threadIdx.x, blk = blockIdx.x, B = gridDim.x;
    const int L = min(kS, F - blk * kS);
    const size_t rec = (size_t)blockIdx.y * B + blk;
    const unsigned char* src = filtered + (size_t)blockIdx.y * filtered_stride + (size_t)blk * kS + tid * kChunk;
    const int count = max(0, min(kChunk, L - tid * kChunk));
    const unsigned st = start[rec];
    const bool stored = (st & kStoredFlag) != 0u;
    const unsigned file_bit = (unsigned)kFileHead * 8u + (st & ~kStoredFlag);
    const unsigned g0 = file_bit >> 5, shift = file_bit & 31u;       // stage[i] is the file's word g0 + i
    const unsigned final_bit = blk == B - 1 ? 1u : 0u;

    for (int i = tid; i < kStageWords; i += kPngThreads) stage[i] = 0;
    for (int s = tid; s < kLenStride; s += kPngThreads) len_of[s] = stored ? 8 : lens[rec * kLenStride + s];
    {                                                     // slicing-by-4 tables: the remainder of byte t followed by k zero bytes
        unsigned v = crc_byte(0u, (unsigned)tid);
        crc_t[0][tid] = v;
#pragma unroll
        for (int k = 1; k < 4; ++k) { v = crc_byte(v, 0u); crc_t[k][tid] = v; }
    }
    __syncthreads();
    for (int s = tid; s < kSyms; s += kPngThreads) {
        const unsigned l = len_of[s];
        unsigned code = (unsigned)s;                      // stored: the byte itself, 8 bits, as it is
        if (!stored && l) {                               // canonical: codes of one length count up in symbol order
            unsigned first = 0, same = 0;
            for (int j = 0; j < kSyms; ++j) {
                const unsigned lj = len_of[j];
                if (lj && lj < l) first += 1u << (l - lj);                 // sum over shorter lengths of count << (l - length)
                same += (lj == l && j < s) ? 1u : 0u;
            }
            code = reverse_bits(first + same, (int)l);
        }
        table[s] = code | (l << 16);
    }
    unsigned w[16];
    load_chunk(src, count, w);
    __syncthreads();
    unsigned nb = 0;
#pragma unroll
    for (int k = 0; k < kChunk; ++k) nb += k < count ? table[chunk_byte(w, k)] >> 16 : 0u;
    scan[tid] = nb;
    __syncthreads();
    for (int d = 1; d < kPngThreads; d <<= 1) {
        const unsigned v = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const unsigned payload_bits = scan[kPngThreads - 1];
    unsigned payload0, end_bit;                           // positions in stage's bit numbering
    if (stored) {
        payload0 = ((shift + 3u + 7u) & ~7u) + 32u;       // the file's byte grid is the stream's
        end_bit = payload0 + payload_bits;
        if (tid == 0) {
            put_bits(stage, shift, final_bit, 3);
            put_bits(stage, payload0 - 32u, (unsigned)L | ((~(unsigned)L & 0xffffu) << 16), 32);
        }
    } else {
        payload0 = shift + kHeaderBits;
        end_bit = payload0 + payload_bits + (table[256] >> 16);
        if (tid == 0) {
            put_bits(stage, shift, final_bit | (2u << 1) | (15u << 13), 17);              // BTYPE 10, HLIT 0, HDIST 0, HCLEN 15
            for (int i = 3; i < 19; ++i) put_bits(stage, shift + 17u + 3u * i, 4u, 3);    // 16 17 18: unused; 0..15: 4 bits
            put_bits(stage, payload0 + payload_bits, table[256] & 0xffffu, (int)(table[256] >> 16));
        }
        for (int s = tid; s < 258; s += kPngThreads)      // 257 literal/length lengths + the one distance length, 0
            put_bits(stage, shift + 74u + 4u * s, reverse_bits(s < kSyms ? len_of[s] : 0u, 4), 4);
    }
    if (count) {
        unsigned pos = payload0 + scan[tid] - nb;
        unsigned wi = pos >> 5, have = pos & 31u;         // the low `have` bits of the first word are someone else's: 0 here
        unsigned long long acc = 0;
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
            if (k < count) {
                const unsigned e = table[chunk_byte(w, k)];
                acc |= (unsigned long long)(e & 0xffffu) << have;
                have += e >> 16;
                if (have >= 32u) {
                    atomicAdd(&stage[wi++], (unsigned)acc);
                    acc >>= 32;
                    have -= 32u;
                }
            }
        }
        if (have) atomicAdd(&stage[wi], (unsigned)acc);
    }
    __syncthreads();

    const unsigned nwords = (end_bit + 31u) >> 5;
    unsigned* words = reinterpret_cast<unsigned*>(out + (size_t)blockIdx.y * out_stride) + g0;
    for (unsigned i = tid; i < nwords; i += kPngThreads) {
        const bool whole = (i > 0 || shift == 0u) && (i + 1 < nwords || (end_bit & 31u) == 0u);
        if (whole) words[i] = stage[i];
        else atomicAdd(&words[i], stage[i]);
    }
    // remainder of stage[0..nwords): thread t takes the kCrcWords words that end (255 - t) * kCrcWords before the end (leading
    // zeros change nothing), then a tree joins neighbours: left * x^(bits of the right part) + right
    unsigned rem = 0;
    const int w0 = (int)nwords - (kPngThreads - tid) * kCrcWords;
    for (int i = max(w0, 0); i < w0 + kCrcWords; ++i) {
        rem ^= stage[i];
        rem = crc_t[3][rem & 255u] ^ crc_t[2][(rem >> 8) & 255u] ^ crc_t[1][(rem >> 16) & 255u] ^ crc_t[0][rem >> 24];
    }
    scan[tid] = rem;
    __syncthreads();
    crc_tree<0>(scan, tid);
    if (tid == 0) {
        crc_rem[rec] = scan[0];
        crc_end[rec] = 4u * (g0 + nwords);
    }
}

// ---- finish --------------------------------------------------------------------------------------------------------------------
// grid (n): the IDAT CRC over type + data = file bytes [37, 47 + deflate bytes)
__global__ __launch_bounds__(256) void png_finish_kernel(const unsigned* __restrict__ crc_rem, const unsigned* __restrict__ crc_end,
                                                         const unsigned* __restrict__ meta, unsigned char* __restrict__ out,
                                                         long long out_stride, int B) {
    __shared__ unsigned red[kPngThreads];
    const int tid = threadIdx.x, img = blockIdx.x;
    const unsigned crc_at = kFileHead + meta[2 * img] + 4u, adler = meta[2 * img + 1];
    unsigned acc = 0;
    for (int k = tid; k < B; k += kPngThreads) {
        const size_t rec = (size_t)img * B + k;
        acc ^= gf_mul(crc_rem[rec], gf_xpow_bytes(crc_at - crc_end[rec]));
    }
    if (tid == 0) {
        const unsigned char head[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
        unsigned r = 0;
        for (int i = 0; i < 6; ++i) r = crc_byte(r, head[i]);
        acc ^= gf_mul(r, gf_xpow_bytes(crc_at - kFileHead));
        r = 0;
        for (int i = 0; i < 4; ++i) r = crc_byte(r, (adler >> (24 - 8 * i)) & 255u);
        acc ^= r;
        acc ^= gf_mul(0xffffffffu, gf_xpow_bytes(crc_at - 37u)) ^ 0xffffffffu;
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = kPngThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] ^= red[tid + s];
        __syncthreads();
    }
    if (tid == 0) put_be32(reinterpret_cast<unsigned*>(out + (size_t)img * out_stride), crc_at, red[0]);
}

}  // namespace clslam

using namespace clslam;

namespace {

struct PngGeometry {
    long long F, blocks, bound;
};

bool png_geometry(int h, int w, int channels, PngGeometry* g) {
    if (h < 1 || w < 1 || (channels != 1 && channels != 3)) return false;
    const long long F = (long long)h * (1 + (long long)w * channels);
    if (F > (1ll << 27)) return false;
    g->F = F;
    g->blocks = (F + kS - 1) / kS;
    g->bound = F + 5 * g->blocks + 63;
    return true;
}

long long round16(long long v) { return (v + 15) & ~15ll; }

// scratch of clslam_png_deflate: per block its code lengths and six words; per image two words
struct PngScratch {
    unsigned char* lens;
    unsigned *dyn_bits, *adler_a, *adler_b, *start, *crc_rem, *crc_end, *meta;
    static long long bytes(long long n, long long blocks) { return round16(n * blocks * (kLenStride + 6 * 4)) + round16(n * 2 * 4); }
    PngScratch(void* base, long long n, long long blocks) {
        const long long recs = n * blocks;
        lens = static_cast<unsigned char*>(base);
        dyn_bits = reinterpret_cast<unsigned*>(lens + recs * kLenStride);
        adler_a = dyn_bits + recs; adler_b = adler_a + recs; start = adler_b + recs; crc_rem = start + recs; crc_end = crc_rem + recs;
        meta = reinterpret_cast<unsigned*>(lens + round16(recs * (kLenStride + 6 * 4)));
    }
};

int png_check_out(const char* fn, const void* out, long long out_stride, const int* lengths, const PngGeometry& g) {
    CLSLAM_REQUIRE(out_stride >= g.bound, "%s: %lld bytes per file, clslam_png_bound is %lld", fn, out_stride, g.bound);
    CLSLAM_REQUIRE(out && lengths && ((size_t)out & 3) == 0 && out_stride % 4 == 0,
                   "%s: null pointer, or out / out_stride not a multiple of 4", fn);
    return CLSLAM_OK;
}

int png_filter_launch(const unsigned char* image, unsigned char* filtered, long long stride, int n, int h, int w, int channels,
                      int filter, hipStream_t stream) {
    hipLaunchKernelGGL(png_filter_kernel, dim3(h, n), dim3(kPngThreads), 0, stream, image, filtered, stride, h, w * channels, channels,
                       filter);
    return check_launch("png_filter");
}

int png_deflate_launch(const unsigned char* filtered, long long stride, unsigned char* out, long long out_stride, int* lengths,
                       void* scratch, int n, int h, int w, int channels, const PngGeometry& g, hipStream_t stream) {
    const PngScratch s(scratch, n, g.blocks);
    const int B = (int)g.blocks, F = (int)g.F;
    const dim3 grid(B, n), block(kPngThreads);
    if (hipMemsetAsync(out, 0, (size_t)n * out_stride, stream) != hipSuccess) {
        set_error("png_deflate: hipMemsetAsync failed");
        return CLSLAM_ERR_INVALID;
    }
    hipLaunchKernelGGL(png_plan_kernel, grid, block, 0, stream, filtered, stride, F, s.lens, s.dyn_bits, s.adler_a, s.adler_b);
    hipLaunchKernelGGL(png_layout_kernel, dim3(n), block, 0, stream, (const unsigned*)s.dyn_bits, (const unsigned*)s.adler_a,
                       (const unsigned*)s.adler_b, s.start, s.meta, out, out_stride, lengths, B, F, h, w, channels);
    hipLaunchKernelGGL(png_pack_kernel, grid, block, 0, stream, filtered, stride, F, (const unsigned char*)s.lens,
                       (const unsigned*)s.start, out, out_stride, s.crc_rem, s.crc_end);
    hipLaunchKernelGGL(png_finish_kernel, dim3(n), block, 0, stream, (const unsigned*)s.crc_rem, (const unsigned*)s.crc_end,
                       (const unsigned*)s.meta, out, out_stride, B);
    return check_launch("png_deflate");
}

}  // namespace

extern "C" long long clslam_png_bound(int h, int w, int channels) {
    PngGeometry g;
    return png_geometry(h, w, channels, &g) ? g.bound : 0;
}

extern "C" long long clslam_png_scratch(int n, int h, int w, int channels) {
    PngGeometry g;
    if (n < 0 || !png_geometry(h, w, channels, &g)) return 0;
    return n * round16(g.F) + PngScratch::bytes(n, g.blocks);
}

#define PNG_GEOMETRY(fn)                                                                                                    \
    PngGeometry g;                                                                                                          \
    CLSLAM_REQUIRE(n >= 0 && n <= 65535, fn ": 0..65535 images per call");                                                  \
    CLSLAM_REQUIRE(png_geometry(h, w, channels, &g), fn ": h, w >= 1, 1 or 3 channels, at most 2^27 filtered bytes per image")

extern "C" int clslam_png_filter(const unsigned char* image, unsigned char* filtered, long long filtered_stride, int n, int h, int w,
                                 int channels, int filter, void* stream_) {
    PNG_GEOMETRY("png_filter");
    CLSLAM_REQUIRE(filter >= CLSLAM_PNG_FILTER_ADAPTIVE && filter <= 4, "png_filter: filter type 0..4 or CLSLAM_PNG_FILTER_ADAPTIVE");
    CLSLAM_REQUIRE(filtered_stride >= g.F, "png_filter: filtered_stride below h * (1 + w * channels)");
    if (n == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(image && filtered, "png_filter: null pointer");
    return png_filter_launch(image, filtered, filtered_stride, n, h, w, channels, filter, (hipStream_t)stream_);
}

extern "C" int clslam_png_deflate(const unsigned char* filtered, long long filtered_stride, unsigned char* out, long long out_stride,
                                  int* lengths, void* scratch, long long scratch_bytes, int n, int h, int w, int channels,
                                  void* stream_) {
    PNG_GEOMETRY("png_deflate");
    CLSLAM_REQUIRE(filtered_stride >= g.F && filtered_stride % 16 == 0, "png_deflate: filtered_stride below h * (1 + w * channels), or not a multiple of 16");
    if (n == 0) return CLSLAM_OK;
    if (int rc = png_check_out("png_deflate", out, out_stride, lengths, g)) return rc;
    CLSLAM_REQUIRE(filtered && ((size_t)filtered & 15) == 0, "png_deflate: filtered null or not 16-byte aligned");
    CLSLAM_REQUIRE(scratch && ((size_t)scratch & 15) == 0 && scratch_bytes >= PngScratch::bytes(n, g.blocks),
                   "png_deflate: scratch null, not 16-byte aligned, or below clslam_png_scratch");
    return png_deflate_launch(filtered, filtered_stride, out, out_stride, lengths, scratch, n, h, w, channels, g, (hipStream_t)stream_);
}

extern "C" int clslam_png_encode(const unsigned char* image, unsigned char* out, long long out_stride, int* lengths, void* scratch,
                                 long long scratch_bytes, int n, int h, int w, int channels, int filter, void* stream_) {
    PNG_GEOMETRY("png_encode");
    CLSLAM_REQUIRE(filter >= CLSLAM_PNG_FILTER_ADAPTIVE && filter <= 4, "png_encode: filter type 0..4 or CLSLAM_PNG_FILTER_ADAPTIVE");
    if (n == 0) return CLSLAM_OK;
    if (int rc = png_check_out("png_encode", out, out_stride, lengths, g)) return rc;
    CLSLAM_REQUIRE(image, "png_encode: null pointer");
    CLSLAM_REQUIRE(scratch && ((size_t)scratch & 15) == 0 && scratch_bytes >= clslam_png_scratch(n, h, w, channels),
                   "png_encode: scratch null, not 16-byte aligned, or below clslam_png_scratch");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned char* filtered = static_cast<unsigned char*>(scratch);
    const long long stride = round16(g.F);
    if (int rc = png_filter_launch(image, filtered, stride, n, h, w, channels, filter, stream)) return rc;
    return png_deflate_launch(filtered, stride, out, out_stride, lengths, filtered + n * stride, n, h, w, channels, g, stream);
}
