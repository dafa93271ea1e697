// apt_kernels_png.hip — PNG encoding on gfx950: scanline filter, per-chunk deflate (hash matcher in
// LDS, greedy parse by pointer doubling, length-limited Huffman codes, bit packing), placement by a scan of the chunk
// sizes, Adler-32 and CRC-32 from per-slice partial values combined on the device.
#include "apt_kernels_png.hpp"

#include <atomic>

namespace apt::png {
namespace {

using apt::gpu::ImageResult;

constexpr int kFilterThreads = 256;
constexpr int kDeflateThreads = 512;
constexpr int kPerThread = kChunk / kDeflateThreads;  // positions of a chunk per lane
constexpr int kHashBits = 12;
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258;
constexpr uint32_t kAdler = 65521;
constexpr uint32_t kPoly = 0xedb88320u;
constexpr int kLitSyms = 286, kDistSyms = 30, kClSyms = 19;
constexpr int kPlaceThreads = 256;
constexpr uint32_t kCrcSlice = 64;  // bytes per lane of the CRC pass
constexpr uint32_t kDataOffset = 8 + 25 + 8 + 2;  // first deflate byte in the file

static_assert(kChunk % kDeflateThreads == 0 && kPerThread == 32, "the parse keeps one mark bit per position in a u32");
static_assert(kChunk <= 32768, "ceil(log2(total / count)) must stay within 15 bits (one symbol per byte + end of block)");

// ws layout
constexpr size_t kCtlBytes = 256;
enum { kCtlOk = 0, kCtlCrc = 1, kCtlDeflate = 2, kCtlChunks = 3 };
struct WsView {
    uint32_t *ctl;
    ChunkRec *recs;
    uint8_t *stream;
    uint8_t *stage;
};
inline size_t align_up(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }
inline WsView carve(void *ws, uint64_t stream_cap)
{
    char *p = static_cast<char *>(ws);
    const uint64_t nc = chunks_of(stream_cap);
    WsView v;
    v.ctl = reinterpret_cast<uint32_t *>(p);
    p += kCtlBytes;
    v.recs = reinterpret_cast<ChunkRec *>(p);
    p += align_up(nc * sizeof(ChunkRec));
    v.stream = reinterpret_cast<uint8_t *>(p);
    p += align_up(stream_cap + 64);
    v.stage = reinterpret_cast<uint8_t *>(p);
    return v;
}

// rows to encode: the image stage's height when a record is given (none when it failed), never past the capacity
__device__ inline uint32_t live_height(const ImageResult *info, uint32_t height)
{
    if (!info) return height;
    if (info->status != 0) return 0;
    return info->height < height ? info->height : height;
}

__device__ inline uint32_t reduce_add_wave(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ------------------------------------------------------------------ 1. scanline filter
__device__ inline int paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ inline uint8_t residual(int f, int v, int a, int b, int c)
{
    switch (f) {
    case 0: return static_cast<uint8_t>(v);
    case 1: return static_cast<uint8_t>(v - a);
    case 2: return static_cast<uint8_t>(v - b);
    case 3: return static_cast<uint8_t>(v - ((a + b) >> 1));
    default: return static_cast<uint8_t>(v - paeth(a, b, c));
    }
}

// One workgroup per row: the filter with the smallest sum of |signed residual| (libpng's heuristic), ties to the lower
// filter number; writes the filter byte and the residuals.
__global__ __launch_bounds__(kFilterThreads) void k_png_filter(const uint8_t *__restrict__ img, uint32_t width,
                                                               uint32_t bpp, const ImageResult *info, uint32_t height,
                                                               uint8_t *__restrict__ stream)
{
    const uint32_t h = live_height(info, height);
    const uint32_t r = blockIdx.x;
    if (r >= h) return;
    __shared__ unsigned long long tot[5];
    __shared__ int chosen;
    if (threadIdx.x < 5) tot[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t rb = static_cast<uint64_t>(width) * bpp;
    const uint8_t *cur = img + r * rb;
    const uint8_t *up = r ? cur - rb : nullptr;
    uint32_t s[5] = {0, 0, 0, 0, 0};
    for (uint64_t x = threadIdx.x; x < rb; x += kFilterThreads) {
        const int v = cur[x];
        const int a = x >= bpp ? cur[x - bpp] : 0;
        const int b = up ? up[x] : 0;
        const int c = (up && x >= bpp) ? up[x - bpp] : 0;
#pragma unroll
        for (int f = 0; f < 5; ++f) s[f] += static_cast<uint32_t>(abs(static_cast<int>(static_cast<int8_t>(residual(f, v, a, b, c)))));
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) {
        const uint32_t w = reduce_add_wave(s[f]);
        if ((threadIdx.x & 63) == 0) atomicAdd(&tot[f], static_cast<unsigned long long>(w));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0;
        for (int f = 1; f < 5; ++f)
            if (tot[f] < tot[best]) best = f;
        chosen = best;
    }
    __syncthreads();
    const int f = chosen;
    uint8_t *dst = stream + r * (rb + 1);
    if (threadIdx.x == 0) dst[0] = static_cast<uint8_t>(f);
    for (uint64_t x = threadIdx.x; x < rb; x += kFilterThreads) {
        const int v = cur[x];
        const int a = x >= bpp ? cur[x - bpp] : 0;
        const int b = up ? up[x] : 0;
        const int c = (up && x >= bpp) ? up[x - bpp] : 0;
        dst[1 + x] = residual(f, v, a, b, c);
    }
}

// ------------------------------------------------------------------ 2. deflate of one chunk
struct DeflateLds {
    uint8_t data[kChunk + 16];
    uint32_t table[1 << kHashBits];  // most recent position + 1 per 4-byte key, 0 = none (earlier strips only)
    uint32_t first[1 << kHashBits];  // earliest position of the current strip per key, ~0 = none
    uint16_t mdist[kChunk];
    union {
        uint16_t jump[kChunk + 8];          // the parse: 2^k-th successor of every position
        uint32_t outw[kChunk / 4 + 8];      // the packed bits (after the parse)
    };
    uint8_t mlen[kChunk];  // match length - 3, 0 = no match
    uint8_t mark[kChunk + 16];
    uint32_t lfreq[288], dfreq[32], clfreq[kClSyms + 1];
    uint16_t lcode[288], dcode[32], clcode[kClSyms + 1];
    uint8_t llen[288], dlen[32], cllen[kClSyms + 1];
    uint16_t lorder[288], dorder[32], clorder[kClSyms + 1];
    uint8_t rle_sym[320], rle_ext[320];
    uint32_t scan[kDeflateThreads];
    uint32_t adler_a, adler_b, header_bits, n_rle;
};
static_assert(sizeof(DeflateLds) <= 160 * 1024, "one chunk must fit the CU's LDS");

__device__ inline uint32_t match_len(const uint8_t *d, uint32_t q, uint32_t p, uint32_t maxlen)
{
    uint32_t l = 0;
    while (l < maxlen && d[q + l] == d[p + l]) ++l;
    return l;
}

__device__ inline void len_code(uint32_t len, uint32_t *code, uint32_t *eb, uint32_t *extra)
{
    if (len == kMaxMatch) {
        *code = 28, *eb = 0, *extra = 0;
        return;
    }
    const uint32_t l = len - 3;
    if (l < 8) {
        *code = l, *eb = 0, *extra = 0;
        return;
    }
    const uint32_t msb = 31u - static_cast<uint32_t>(__clz(static_cast<int>(l)));
    *eb = msb - 2;
    *code = 4 * *eb + 4 + ((l >> *eb) & 3u);
    *extra = l & ((1u << *eb) - 1u);
}

__device__ inline void dist_code(uint32_t dist, uint32_t *code, uint32_t *eb, uint32_t *extra)
{
    const uint32_t d = dist - 1;
    if (d < 4) {
        *code = d, *eb = 0, *extra = 0;
        return;
    }
    const uint32_t msb = 31u - static_cast<uint32_t>(__clz(static_cast<int>(d)));
    *eb = msb - 1;
    *code = 2 * msb + ((d >> (msb - 1)) & 1u);
    *extra = d & ((1u << *eb) - 1u);
}

// order[rank] = symbol, by descending count, ties to the lower symbol; one lane per symbol
__device__ inline void rank_sort(const uint32_t *freq, int n, int s, uint16_t *order)
{
    const uint32_t f = freq[s];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const uint32_t g = freq[j];
        rank += (g > f || (g == f && j < s)) ? 1 : 0;
    }
    order[rank] = static_cast<uint16_t>(s);
}

// Code lengths of at most `limit` bits for the symbols with a count (at least two of them), by one lane: every
// symbol starts at ceil(log2(total / count)) clipped to the limit, the rarest are lengthened while the Kraft sum is
// above one (only the clipping can cause that), then the most frequent are shortened while there is room.  The last
// pass leaves no room, so the code is complete, as inflate demands.
__device__ void build_lengths(const uint32_t *freq, int n, int limit, const uint16_t *order, uint8_t *len)
{
    uint32_t total = 0;
    for (int i = 0; i < n; ++i) total += freq[i];
    const int one = 1 << limit;
    int kraft = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t f = freq[i];
        int l = 0;
        if (f) {
            l = 1;
            while (l < limit && (static_cast<uint64_t>(f) << l) < total) ++l;
            kraft += one >> l;
        }
        len[i] = static_cast<uint8_t>(l);
    }
    while (kraft > one) {
        for (int r = n - 1; r >= 0; --r) {
            const int s = order[r];
            if (freq[s] && len[s] < limit) {
                kraft -= one >> (len[s] + 1);
                ++len[s];
                break;
            }
        }
    }
    int room = one - kraft;
    for (int r = 0; r < n; ++r) {
        const int s = order[r];
        if (!freq[s]) break;
        while (len[s] > 1 && (one >> len[s]) <= room) {
            room -= one >> len[s];
            --len[s];
        }
    }
}

// canonical code of symbol s (RFC 1951 §3.2.2), bit-reversed for the LSB-first stream; one lane per symbol
__device__ inline uint16_t canonical_code(const uint8_t *len, int n, int s)
{
    const int l = len[s];
    if (!l) return 0;
    uint32_t code = 0;
    for (int j = 0; j < n; ++j) {
        const int lj = len[j];
        if (lj && lj < l) code += 1u << (l - lj);
        else if (lj == l && j < s) code += 1u;
    }
    return static_cast<uint16_t>(__brev(code) >> (32 - l));
}

// ORs the low nb (<= 48) bits of val into the stream at bit `pos`
__device__ inline void put_bits(uint32_t *outw, uint32_t pos, uint64_t val, uint32_t nb)
{
    if (!nb) return;
    const uint32_t w = pos >> 5, sh = pos & 31u;
    const uint64_t lo = val << sh;
    const uint32_t hi = sh ? static_cast<uint32_t>(val >> (64 - sh)) : 0u;
    if (static_cast<uint32_t>(lo)) atomicOr(&outw[w], static_cast<uint32_t>(lo));
    if (static_cast<uint32_t>(lo >> 32)) atomicOr(&outw[w + 1], static_cast<uint32_t>(lo >> 32));
    if (hi) atomicOr(&outw[w + 2], hi);
}

// The dynamic block's header by one lane: HLIT / HDIST, the run-length coded lengths, their 7-bit code.  Returns its
// size in bits (BFINAL = 0, BTYPE = 10 included).
__device__ uint32_t write_header(DeflateLds &L)
{
    int hlit = kLitSyms, hdist = kDistSyms;
    while (hlit > 257 && L.llen[hlit - 1] == 0) --hlit;
    while (hdist > 1 && L.dlen[hdist - 1] == 0) --hdist;
    const int n = hlit + hdist;
    auto at = [&](int i) -> int { return i < hlit ? L.llen[i] : L.dlen[i - hlit]; };
    for (int i = 0; i <= kClSyms; ++i) L.clfreq[i] = 0;
    int m = 0;
    auto emit = [&](int sym, int ext) {
        L.rle_sym[m] = static_cast<uint8_t>(sym);
        L.rle_ext[m] = static_cast<uint8_t>(ext);
        ++m;
        ++L.clfreq[sym];
    };
    for (int i = 0; i < n;) {
        const int v = at(i);
        int run = 1;
        while (i + run < n && at(i + run) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                emit(18, r - 11);
                run -= r;
            }
            if (run >= 3) {
                emit(17, run - 3);
                run = 0;
            }
            for (; run > 0; --run) emit(0, 0);
        } else {
            emit(v, 0);
            --run;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                emit(16, r - 3);
                run -= r;
            }
            for (; run > 0; --run) emit(v, 0);
        }
    }
    int used = 0, first = -1;
    for (int i = 0; i < kClSyms; ++i)
        if (L.clfreq[i]) {
            ++used;
            if (first < 0) first = i;
        }
    if (used < 2) L.clfreq[first == 0 ? 1 : 0] = 1;  // (a complete code needs two symbols)
    for (int s = 0; s < kClSyms; ++s) rank_sort(L.clfreq, kClSyms, s, L.clorder);
    build_lengths(L.clfreq, kClSyms, 7, L.clorder, L.cllen);
    for (int s = 0; s < kClSyms; ++s) L.clcode[s] = canonical_code(L.cllen, kClSyms, s);
    const int perm[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = kClSyms;
    while (hclen > 4 && L.cllen[perm[hclen - 1]] == 0) --hclen;
    uint32_t pos = 0;
    auto put = [&](uint32_t v, uint32_t nb) {
        put_bits(L.outw, pos, v, nb);
        pos += nb;
    };
    put(0, 1);  // BFINAL: the chunk's last block is the empty stored one
    put(2, 2);  // BTYPE = 10, dynamic
    put(static_cast<uint32_t>(hlit - 257), 5);
    put(static_cast<uint32_t>(hdist - 1), 5);
    put(static_cast<uint32_t>(hclen - 4), 4);
    for (int i = 0; i < hclen; ++i) put(L.cllen[perm[i]], 3);
    for (int i = 0; i < m; ++i) {
        const int s = L.rle_sym[i];
        put(L.clcode[s], L.cllen[s]);
        if (s == 16) put(L.rle_ext[i], 2);
        else if (s == 17) put(L.rle_ext[i], 3);
        else if (s == 18) put(L.rle_ext[i], 7);
    }
    return pos;
}

// bits of the token that starts at position i (0 when none does); with `val` also the bits themselves
__device__ inline uint32_t token_bits(const DeflateLds &L, uint32_t i, bool marked, uint64_t *val)
{
    if (!marked) return 0;
    const uint32_t ml = L.mlen[i];
    if (!ml) {
        const uint32_t b = L.data[i];
        if (val) *val = L.lcode[b];
        return L.llen[b];
    }
    uint32_t lc, leb, lex, dc, deb, dex;
    len_code(ml + 3, &lc, &leb, &lex);
    dist_code(L.mdist[i], &dc, &deb, &dex);
    const uint32_t ls = 257 + lc;
    uint32_t nb = L.llen[ls];
    if (val) {
        uint64_t v = L.lcode[ls];
        v |= static_cast<uint64_t>(lex) << nb;
        v |= static_cast<uint64_t>(L.dcode[dc]) << (nb + leb);
        v |= static_cast<uint64_t>(dex) << (nb + leb + L.dlen[dc]);
        *val = v;
    }
    return nb + leb + L.dlen[dc] + deb;
}

// One workgroup per chunk of the filtered stream: match, parse, code, pack into the chunk's staging area.
__global__ __launch_bounds__(kDeflateThreads) void k_png_deflate(const uint8_t *__restrict__ stream, uint32_t width,
                                                                 uint32_t bpp, const ImageResult *info, uint32_t height,
                                                                 ChunkRec *__restrict__ recs, uint8_t *__restrict__ stage)
{
    extern __shared__ __align__(16) unsigned char smem[];
    DeflateLds &L = *reinterpret_cast<DeflateLds *>(smem);
    const uint64_t total = static_cast<uint64_t>(live_height(info, height)) * (static_cast<uint64_t>(width) * bpp + 1u);
    const uint64_t chunk = blockIdx.x;
    if (chunk * kChunk >= total) return;
    const uint32_t n = static_cast<uint32_t>(total - chunk * kChunk < kChunk ? total - chunk * kChunk : kChunk);
    const bool last = (chunk + 1) * kChunk >= total;
    const uint32_t tid = threadIdx.x;
    const uint8_t *src = stream + chunk * kChunk;

    // load (the chunk starts 4-byte aligned), clear the tables
    for (uint32_t i = tid * 4; i + 4 <= n; i += kDeflateThreads * 4)
        *reinterpret_cast<uint32_t *>(&L.data[i]) = *reinterpret_cast<const uint32_t *>(&src[i]);
    if ((n & ~3u) + tid < n) L.data[(n & ~3u) + tid] = src[(n & ~3u) + tid];
    if (tid < 16) L.data[n + tid] = 0;
    for (uint32_t i = tid; i < (1u << kHashBits); i += kDeflateThreads) L.table[i] = 0;
    for (uint32_t i = tid; i < kChunk + 16; i += kDeflateThreads) L.mark[i] = 0;
    if (tid < 288) L.lfreq[tid] = tid == 256 ? 1u : 0u;
    if (tid < 32) L.dfreq[tid] = 0;
    if (tid == 0) L.adler_a = L.adler_b = 0;
    __syncthreads();

    // Adler-32 partial sums of the chunk: a = sum d, b = sum (n - j) d_j
    {
        uint32_t a = 0, b = 0;
        const uint32_t j0 = tid * kPerThread;
        for (uint32_t k = 0; k < kPerThread; ++k) {
            const uint32_t j = j0 + k;
            if (j < n) {
                const uint32_t d = L.data[j];
                a += d;
                b += (n - j) * d;
            }
        }
        a = reduce_add_wave(a % kAdler);
        b = reduce_add_wave(b % kAdler);
        if ((tid & 63u) == 0) {
            atomicAdd(&L.adler_a, a);
            atomicAdd(&L.adler_b, b);
        }
    }

    // matches, strip by strip.  A lane sees the earlier strips through `table` (most recent position per key) and
    // its own strip through `first` (the strip's earliest position per key); the longer match wins, then the nearer.
    for (uint32_t base = 0; base < n; base += kDeflateThreads) {
        const uint32_t p = base + tid;
        uint32_t best = 0, bdist = 0, hsh = 0;
        const bool key = p + kMinMatch <= n;
        if (key) {
            const uint32_t k4 = L.data[p] | (L.data[p + 1] << 8) | (L.data[p + 2] << 16) |
                                (static_cast<uint32_t>(L.data[p + 3]) << 24);
            hsh = (k4 * 2654435761u) >> (32 - kHashBits);
        }
        for (uint32_t i = tid; i < (1u << kHashBits); i += kDeflateThreads) L.first[i] = 0xffffffffu;
        __syncthreads();  // (also: the previous strip's entries are in `table`)
        if (key) atomicMin(&L.first[hsh], p);
        __syncthreads();
        if (key) {
            const uint32_t maxlen = n - p < kMaxMatch ? n - p : kMaxMatch;
            uint32_t cand[3];
            cand[0] = p >= bpp ? p - bpp : p;  // the previous pixel
            const uint32_t c = L.table[hsh];
            cand[1] = c ? c - 1 : p;
            const uint32_t e = L.first[hsh];
            cand[2] = e < p ? e : p;
            for (int k = 0; k < 3; ++k) {
                const uint32_t q = cand[k];
                if (q >= p || p - q == bdist || best == maxlen) continue;
                const uint32_t l = match_len(L.data, q, p, maxlen);
                if (l >= kMinMatch && (l > best || (l == best && p - q < bdist))) best = l, bdist = p - q;
            }
        }
        if (p < n) {
            L.mlen[p] = static_cast<uint8_t>(best ? best - 3 : 0);
            L.mdist[p] = static_cast<uint16_t>(bdist);
        }
        __syncthreads();
        if (key) atomicMax(&L.table[hsh], p + 1);  // the most recent position wins, whatever the lane order
    }
    __syncthreads();

    // greedy parse: the positions reachable from 0 over next[i] = i + len, by pointer doubling
    for (uint32_t i = tid; i <= n; i += kDeflateThreads) {
        const uint32_t step = i < n ? (L.mlen[i] ? L.mlen[i] + 3u : 1u) : 0u;
        L.jump[i] = static_cast<uint16_t>(i + step);
    }
    if (tid == 0) L.mark[0] = 1;
    __syncthreads();
    {
        const int rounds = 32 - __clz(static_cast<int>(n));  // 2^rounds > n - 1 steps
        uint32_t jj[kPerThread];
        for (int r = 0; r < rounds; ++r) {
            uint32_t mk = 0;
#pragma unroll
            for (int k = 0; k < kPerThread; ++k) {
                const uint32_t i = tid + static_cast<uint32_t>(k) * kDeflateThreads;
                if (i < n) {
                    const uint32_t j = L.jump[i];
                    jj[k] = j | (static_cast<uint32_t>(L.jump[j]) << 16);
                    mk |= static_cast<uint32_t>(L.mark[i]) << k;
                } else {
                    jj[k] = 0;
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kPerThread; ++k) {
                const uint32_t i = tid + static_cast<uint32_t>(k) * kDeflateThreads;
                if (i < n) {
                    if ((mk >> k) & 1u) L.mark[jj[k] & 0xffffu] = 1;
                    L.jump[i] = static_cast<uint16_t>(jj[k] >> 16);
                }
            }
            __syncthreads();
        }
    }

    // the tokens' symbol counts (the end-of-block symbol is already in)
    const uint32_t i0 = tid * kPerThread;
    uint32_t mybits = 0;
    for (uint32_t k = 0; k < kPerThread; ++k) {
        const uint32_t i = i0 + k;
        if (i < n && L.mark[i]) {
            mybits |= 1u << k;
            const uint32_t ml = L.mlen[i];
            if (!ml) {
                atomicAdd(&L.lfreq[L.data[i]], 1u);
            } else {
                uint32_t lc, leb, lex, dc, deb, dex;
                len_code(ml + 3, &lc, &leb, &lex);
                dist_code(L.mdist[i], &dc, &deb, &dex);
                atomicAdd(&L.lfreq[257 + lc], 1u);
                atomicAdd(&L.dfreq[dc], 1u);
            }
        }
    }
    __syncthreads();  // (the parse is done: jump's bytes become outw)
    for (uint32_t i = tid; i < kChunk / 4 + 8; i += kDeflateThreads) L.outw[i] = 0;
    if (tid == 0) {  // a complete distance code needs two symbols
        int used = 0;
        for (int s = 0; s < kDistSyms; ++s) used += L.dfreq[s] ? 1 : 0;
        if (used == 0) L.dfreq[0] = L.dfreq[1] = 1;
        else if (used == 1) L.dfreq[L.dfreq[0] ? 1 : 0] = 1;
    }
    __syncthreads();
    if (tid < kLitSyms) rank_sort(L.lfreq, kLitSyms, static_cast<int>(tid), L.lorder);
    else if (tid >= 320 && tid < 320 + kDistSyms) rank_sort(L.dfreq, kDistSyms, static_cast<int>(tid) - 320, L.dorder);
    __syncthreads();
    if (tid == 0) build_lengths(L.lfreq, kLitSyms, 15, L.lorder, L.llen);
    else if (tid == 64) build_lengths(L.dfreq, kDistSyms, 15, L.dorder, L.dlen);
    __syncthreads();
    if (tid < kLitSyms) L.lcode[tid] = canonical_code(L.llen, kLitSyms, static_cast<int>(tid));
    else if (tid >= 320 && tid < 320 + kDistSyms) L.dcode[tid - 320] = canonical_code(L.dlen, kDistSyms, static_cast<int>(tid) - 320);
    __syncthreads();
    if (tid == 0) L.header_bits = write_header(L);

    // bit offsets of the tokens: a scan over the lanes' totals
    uint32_t mine = 0;
    for (uint32_t k = 0; k < kPerThread; ++k) mine += token_bits(L, i0 + k, (mybits >> k) & 1u, nullptr);
    L.scan[tid] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < kDeflateThreads; off <<= 1) {
        const uint32_t t = tid >= off ? L.scan[tid - off] : 0u;
        __syncthreads();
        L.scan[tid] += t;
        __syncthreads();
    }
    const uint32_t token_total = L.scan[kDeflateThreads - 1];
    const uint32_t end_pos = L.header_bits + token_total;  // where the end-of-block code goes
    const uint32_t tail_pos = end_pos + L.llen[256];         // the empty stored block that byte-aligns the chunk
    const uint32_t dyn_bytes = (tail_pos + 3 + 7) / 8 + 4;
    const bool dynamic = dyn_bytes < n + 5;
    uint8_t *dst = stage + chunk * kStageStride;
    uint32_t out_bytes;
    if (dynamic) {
        uint32_t pos = L.header_bits + L.scan[tid] - mine;
        for (uint32_t k = 0; k < kPerThread; ++k) {
            uint64_t v = 0;
            const uint32_t nb = token_bits(L, i0 + k, (mybits >> k) & 1u, &v);
            put_bits(L.outw, pos, v, nb);
            pos += nb;
        }
        if (tid == 0) {
            put_bits(L.outw, end_pos, L.lcode[256], L.llen[256]);
            put_bits(L.outw, tail_pos, last ? 1u : 0u, 3);  // BFINAL, BTYPE = 00; LEN = 0 stays zero
            const uint32_t len_byte = (tail_pos + 3 + 7) / 8;
            put_bits(L.outw, (len_byte + 2) * 8, 0xffffu, 16);  // NLEN
        }
        __syncthreads();
        out_bytes = dyn_bytes;
        uint32_t *dw = reinterpret_cast<uint32_t *>(dst);
        for (uint32_t w = tid; w < (dyn_bytes + 3) / 4; w += kDeflateThreads) dw[w] = L.outw[w];
    } else {
        out_bytes = n + 5;
        if (tid == 0) {
            dst[0] = last ? 1 : 0;
            dst[1] = static_cast<uint8_t>(n & 0xffu);
            dst[2] = static_cast<uint8_t>(n >> 8);
            dst[3] = static_cast<uint8_t>(~n & 0xffu);
            dst[4] = static_cast<uint8_t>((~n >> 8) & 0xffu);
        }
        for (uint32_t i = tid; i < n; i += kDeflateThreads) dst[5 + i] = L.data[i];
    }
    if (tid == 0) recs[chunk] = ChunkRec{out_bytes, L.adler_a % kAdler, L.adler_b % kAdler, 0u};
}

// ------------------------------------------------------------------ 3. layout, placement, checksums
// multiplication modulo the CRC-32 polynomial, reflected bit order (x^0 = bit 31), a != 0 not required
__device__ inline uint32_t multmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}

// x2n[k] = x^(2^k) mod p
__device__ inline void x2n_fill(uint32_t *x2n)
{
    uint32_t p = 1u << 30;  // x^1
    x2n[0] = p;
    for (int k = 1; k < 32; ++k) x2n[k] = p = multmodp(p, p);
}

// x^(8 n) mod p
__device__ inline uint32_t x8n(const uint32_t *x2n, uint64_t n)
{
    uint32_t p = 1u << 31;
    for (uint32_t k = 3; n; n >>= 1, ++k)
        if (n & 1u) p = multmodp(x2n[k & 31u], p);
    return p;
}

__device__ inline uint32_t crc_bitwise(uint32_t c, uint8_t b)
{
    c ^= b;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
    return c;
}

__device__ inline void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = static_cast<uint8_t>(v >> 24);
    p[1] = static_cast<uint8_t>(v >> 16);
    p[2] = static_cast<uint8_t>(v >> 8);
    p[3] = static_cast<uint8_t>(v);
}

constexpr int kLayoutThreads = 1024;

// One workgroup: exclusive scan of the chunk sizes, Adler-32 of the whole stream, the capacity check, the fixed
// chunks.  Leaves ctl for the placement.
__global__ __launch_bounds__(kLayoutThreads) void k_png_layout(ChunkRec *recs, uint32_t *ctl, uint32_t width, uint32_t bpp,
                                                               ImageResult *info, uint32_t height, uint8_t *png,
                                                               uint64_t png_cap, uint64_t *d_len)
{
    __shared__ uint32_t part[kLayoutThreads];
    __shared__ unsigned long long sum_a, sum_b;
    __shared__ uint32_t carry;
    const uint32_t tid = threadIdx.x;
    const uint32_t h = live_height(info, height);
    const uint64_t total = static_cast<uint64_t>(h) * (static_cast<uint64_t>(width) * bpp + 1u);
    const uint32_t nch = static_cast<uint32_t>((total + kChunk - 1) / kChunk);
    if (nch == 0) {
        if (tid == 0) {
            ctl[kCtlOk] = 0;
            ctl[kCtlChunks] = 0;
            if (info) info->reserved = 0;
            if (d_len) *d_len = 0;
        }
        return;
    }
    if (tid == 0) sum_a = sum_b = 0, carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nch; base += kLayoutThreads) {
        const uint32_t i = base + tid;
        ChunkRec rc{0, 0, 0, 0};
        if (i < nch) rc = recs[i];
        part[tid] = rc.bytes;
        __syncthreads();
        for (uint32_t off = 1; off < kLayoutThreads; off <<= 1) {
            const uint32_t t = tid >= off ? part[tid - off] : 0u;
            __syncthreads();
            part[tid] += t;
            __syncthreads();
        }
        if (i < nch) {
            recs[i].offset = carry + part[tid] - rc.bytes;
            const uint64_t end = static_cast<uint64_t>(i + 1) * kChunk;
            const uint64_t after = end < total ? total - end : 0;
            atomicAdd(&sum_a, static_cast<unsigned long long>(rc.adler_a));
            atomicAdd(&sum_b, static_cast<unsigned long long>((rc.adler_b + (after % kAdler) * rc.adler_a) % kAdler));
        }
        __syncthreads();
        if (tid == 0) carry += part[kLayoutThreads - 1];
        __syncthreads();
    }
    if (tid != 0) return;
    const uint32_t deflate = carry;
    const uint64_t file_len = static_cast<uint64_t>(deflate) + 63u;
    const bool ok = file_len <= png_cap;
    ctl[kCtlOk] = ok ? 1u : 0u;
    ctl[kCtlCrc] = 0;
    ctl[kCtlDeflate] = deflate;
    ctl[kCtlChunks] = nch;
    if (d_len) *d_len = file_len;
    if (info) {
        info->reserved = file_len > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(file_len);
        if (!ok) {
            info->status = 1;
            info->reason = kReasonCapacity;
        }
    }
    if (!ok) return;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (int i = 0; i < 8; ++i) png[i] = sig[i];
    uint8_t *p = png + 8;
    put_be32(p, 13);
    p[4] = 'I', p[5] = 'H', p[6] = 'D', p[7] = 'R';
    put_be32(p + 8, width);
    put_be32(p + 12, h);
    p[16] = 8;
    p[17] = bpp == 4 ? 6 : 0;
    p[18] = p[19] = p[20] = 0;
    uint32_t c = 0xffffffffu;
    for (int i = 4; i < 21; ++i) c = crc_bitwise(c, p[i]);
    put_be32(p + 21, c ^ 0xffffffffu);
    p = png + 33;
    put_be32(p, deflate + 6u);
    p[4] = 'I', p[5] = 'D', p[6] = 'A', p[7] = 'T';
    p[8] = 0x78, p[9] = 0x9c;  // deflate, 32 KiB window; FLG makes the pair a multiple of 31
    const uint32_t a = static_cast<uint32_t>((1u + sum_a) % kAdler);
    const uint32_t b = static_cast<uint32_t>((total % kAdler + sum_b) % kAdler);
    uint8_t *q = png + kDataOffset + deflate;
    put_be32(q, (b << 16) | a);
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) q[8 + i] = iend[i];
}

// One workgroup per chunk: its bytes go to their place; the CRC-32 of every 64-byte slice, times x^(8 * bytes behind
// it in IDAT) mod p, is folded into ctl (exclusive or: any order gives the same value).
__global__ __launch_bounds__(kPlaceThreads) void k_png_place(const ChunkRec *__restrict__ recs, uint32_t *ctl,
                                                             const uint8_t *__restrict__ stage, uint8_t *__restrict__ png)
{
    __shared__ uint32_t buf[kStageStride / 4];
    __shared__ uint32_t tab[256];
    __shared__ uint32_t x2n[32];
    __shared__ uint32_t acc;
    const uint32_t chunk = blockIdx.x, tid = threadIdx.x;
    if (!ctl[kCtlOk] || chunk >= ctl[kCtlChunks]) return;
    const ChunkRec rc = recs[chunk];
    const uint32_t deflate = ctl[kCtlDeflate];
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(stage + static_cast<uint64_t>(chunk) * kStageStride);
    for (uint32_t w = tid; w < (rc.bytes + 3) / 4; w += kPlaceThreads) buf[w] = sw[w];
    {
        uint32_t c = tid;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
        tab[tid] = c;
    }
    if (tid == 0) {
        x2n_fill(x2n);
        acc = 0;
    }
    __syncthreads();
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(buf);
    uint8_t *dst = png + kDataOffset + rc.offset;
    for (uint32_t i = tid; i < rc.bytes; i += kPlaceThreads) dst[i] = bytes[i];
    uint32_t term = 0;
    for (uint32_t s0 = tid * kCrcSlice; s0 < rc.bytes; s0 += kPlaceThreads * kCrcSlice) {
        const uint32_t s1 = s0 + kCrcSlice < rc.bytes ? s0 + kCrcSlice : rc.bytes;
        uint32_t c = 0xffffffffu;
        for (uint32_t i = s0; i < s1; ++i) c = tab[(c ^ bytes[i]) & 0xffu] ^ (c >> 8);
        c ^= 0xffffffffu;
        const uint64_t after = static_cast<uint64_t>(deflate) + 4u - (static_cast<uint64_t>(rc.offset) + s1);
        term ^= multmodp(x8n(x2n, after), c);
    }
    for (int o = 32; o > 0; o >>= 1) term ^= __shfl_down(term, o, 64);
    if ((tid & 63u) == 0 && term) atomicXor(&acc, term);
    __syncthreads();
    if (tid == 0 && acc) atomicXor(&ctl[kCtlCrc], acc);
}

// IDAT's CRC: the chunks' part from ctl, "IDAT" + the zlib header in front, the Adler-32 value behind.
__global__ void k_png_finish(const uint32_t *ctl, uint8_t *png)
{
    if (threadIdx.x != 0 || blockIdx.x != 0 || !ctl[kCtlOk]) return;
    uint32_t x2n[32];
    x2n_fill(x2n);
    const uint32_t deflate = ctl[kCtlDeflate];
    uint32_t head = 0xffffffffu, tail = 0xffffffffu;
    for (int i = 0; i < 6; ++i) head = crc_bitwise(head, png[37 + i]);
    const uint8_t *q = png + kDataOffset + deflate;
    for (int i = 0; i < 4; ++i) tail = crc_bitwise(tail, q[i]);
    head ^= 0xffffffffu;
    tail ^= 0xffffffffu;
    const uint32_t crc = multmodp(x8n(x2n, static_cast<uint64_t>(deflate) + 4u), head) ^ ctl[kCtlCrc] ^ tail;
    put_be32(png + kDataOffset + deflate + 4, crc);
}

void allow_lds()
{
    // hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of the function: set it once per device
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    apt::hip_check(hipGetDevice(&dev), "hipGetDevice");
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return;
    apt::hip_check(hipFuncSetAttribute(reinterpret_cast<const void *>(k_png_deflate),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(sizeof(DeflateLds))),
                   "hipFuncSetAttribute (k_png_deflate)");
    done.fetch_or(bit, std::memory_order_release);
}

}  // namespace

size_t ws_bytes(uint64_t stream_cap)
{
    const uint64_t nc = chunks_of(stream_cap);
    return kCtlBytes + align_up(nc * sizeof(ChunkRec)) + align_up(stream_cap + 64) + align_up(nc * kStageStride);
}

void encode_filter(hipStream_t s, const uint8_t *img, uint32_t width, uint32_t height, int channels, void *ws,
                   uint64_t stream_cap, const apt::gpu::ImageResult *info)
{
    if (height == 0) return;
    const WsView v = carve(ws, stream_cap);
    hipLaunchKernelGGL(k_png_filter, dim3(height), dim3(kFilterThreads), 0, s, img, width,
                       static_cast<uint32_t>(channels), info, height, v.stream);
}

void encode_deflate(hipStream_t s, uint32_t width, uint32_t height, int channels, void *ws, uint64_t stream_cap,
                    const apt::gpu::ImageResult *info)
{
    const uint64_t nc = chunks_of(stream_bytes(width, height, channels));
    if (nc == 0) return;
    allow_lds();
    const WsView v = carve(ws, stream_cap);
    hipLaunchKernelGGL(k_png_deflate, dim3(static_cast<unsigned>(nc)), dim3(kDeflateThreads), sizeof(DeflateLds), s,
                       v.stream, width, static_cast<uint32_t>(channels), info, height, v.recs, v.stage);
}

void encode_place(hipStream_t s, uint32_t width, uint32_t height, int channels, void *ws, uint64_t stream_cap,
                  uint8_t *d_png, uint64_t png_cap, apt::gpu::ImageResult *info, uint64_t *d_len)
{
    const uint64_t nc = chunks_of(stream_bytes(width, height, channels));
    const WsView v = carve(ws, stream_cap);
    hipLaunchKernelGGL(k_png_layout, dim3(1), dim3(kLayoutThreads), 0, s, v.recs, v.ctl, width,
                       static_cast<uint32_t>(channels), info, height, d_png, png_cap, d_len);
    if (nc == 0) return;
    hipLaunchKernelGGL(k_png_place, dim3(static_cast<unsigned>(nc)), dim3(kPlaceThreads), 0, s, v.recs, v.ctl, v.stage,
                       d_png);
    hipLaunchKernelGGL(k_png_finish, dim3(1), dim3(64), 0, s, v.ctl, d_png);
}

void encode(hipStream_t s, const uint8_t *img, uint32_t width, uint32_t height, int channels, void *ws,
            uint64_t stream_cap, uint8_t *d_png, uint64_t png_cap, apt::gpu::ImageResult *info, uint64_t *d_len)
{
    encode_filter(s, img, width, height, channels, ws, stream_cap, info);
    encode_deflate(s, width, height, channels, ws, stream_cap, info);
    encode_place(s, width, height, channels, ws, stream_cap, d_png, png_cap, info, d_len);
}

}  // namespace apt::png
