// Block container of encoded.dat: the host-side steps on either side of the GPU kernels.
//
//   split_encoded_dictionary  encode.rs:168-229  (4 streams: colex ranks, match lengths,
//                                                 flag bytes, short-record bases in 31-base
//                                                 as_2bit chunks)
//   rice_encode / minimal_binary_encode         encode.rs:59-94   [ext dsi-bitstream 0.5.0]
//   deflate_bytes (gzip, level 6)               encode.rs:49-57   [ext flate2 1.1.2]
//   compress_block + BlockHeader (32 B)         encode.rs:96-127, lib.rs:37-50,75-86
//   write_block_to                              lib.rs:232-252
//   decode_block / decompress_block /
//   zip_block_contents                          lib.rs:320-368, decode.rs:41-149
//   file header (4 x u64 = 32 zero bytes)       lib.rs:29-35,52-73
//
// write_block_to = pack (everything before deflate: ntc_pack_block here, or the GPU packer
// ntc_pack_blocks_device in pack.hip) + deflate (ntc_deflate_block).  The packed streams
// are pinned by tests/golden/make_codec_golden.py, an independent restatement.
//
// Restated dsi-bitstream semantics (not in the container; recalled):
//   * BufBitWriter<BE, u64 words>: bits MSB-first into u64 words, last word zero-padded;
//     the writer hands words over as to_be(), encode.rs:107-109 emits to_ne_bytes
//     (little-endian): on disk each word is big-endian, i.e. the MSB-first bit stream.
//   * unary(n) = n zeros then a one; rice(n, b) = unary(n >> b) then the low b bits.
//   * rice::log2_b(p) = ceil(log2(ln(phi) / -ln(1-p))), saturating at 0 (Rust `as usize`).
//   * minimal_binary(v, max): l = floor(log2 max), limit = 2^(l+1) - max;
//     v < limit -> v in l bits, else v + limit in l+1 bits.
//   * gzip member like flate2's GzEncoder: 10-byte header (mtime 0, XFL 0, OS 255), raw
//     deflate at level 6, CRC32 + ISIZE trailer.  Deflate bytes come from system zlib (or
//     libdeflate), so they inflate identically but are not byte-identical to zlib-rs
//     (parity level F is unpinned).
#include <dlfcn.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ntcomp_codec.h"
#include "../../include/ntcomp_host.h"
#include "ntc_internal.h"
#include "codec_params.h"
#include "nonacgt_core.h"
#include "qrans_core.h"
#include "quality_core.h"
#include "names_core.h"
#include "digest_core.h"
#include "deflate_core.h"

namespace {

// ---- bit writer / reader (big-endian bit order in u64 words) -------------------------
// Writes into a caller-sized word array (exact sizes come from a counting pass).
struct BitSink {
    uint64_t *w;
    uint64_t n = 0;    // complete words written
    uint64_t acc = 0;  // bits in progress, from the MSB
    int used = 0;      // 0..63
    explicit BitSink(uint64_t *words) : w(words) {}
    inline void put(uint64_t v, int nb) {  // v < 2^nb, nb <= 64
        if (nb <= 0) return;
        const int room = 64 - used;
        if (nb < room) {
            acc |= v << (room - nb);
            used += nb;
        } else {
            const int lo = nb - room;  // 0..63 bits spill into the next word
            w[n++] = acc | (lo ? v >> lo : v);
            acc = lo ? v << (64 - lo) : 0;
            used = lo;
        }
    }
    inline void zeros(uint64_t z) {  // z zero bits
        uint64_t t = (uint64_t)used + z;
        if (t >= 64) {
            w[n++] = acc;
            acc = 0;
            t -= 64;
            while (t >= 64) {
                w[n++] = 0;
                t -= 64;
            }
        }
        used = (int)t;
    }
    uint64_t finish() {
        if (used) {
            w[n++] = acc;
            acc = 0;
            used = 0;
        }
        return n;
    }
};

struct BitReader {
    const uint64_t *w;
    uint64_t nw, pos = 0;  // bit position
    BitReader(const uint64_t *words, uint64_t n) : w(words), nw(n) {}
    // the next 64 bits from pos, MSB first (zero past the end)
    uint64_t peek64() const {
        const uint64_t i = pos >> 6, sh = pos & 63;
        const uint64_t hi = i < nw ? w[i] : 0;
        if (!sh) return hi;
        const uint64_t lo = i + 1 < nw ? w[i + 1] : 0;
        return (hi << sh) | (lo >> (64 - sh));
    }
    bool bit(int &b) {
        if (pos >= nw * 64) return false;
        b = (int)((w[pos >> 6] >> (63 - (pos & 63))) & 1);
        pos++;
        return true;
    }
    bool get(int nbits, uint64_t &v) {
        if (nbits == 0) {
            v = 0;
            return true;
        }
        if (pos + (uint64_t)nbits > nw * 64) return false;
        v = peek64() >> (64 - nbits);
        pos += (uint64_t)nbits;
        return true;
    }
    bool unary(uint64_t &n) {  // zeros up to and including the terminating one
        n = 0;
        for (;;) {
            if (pos >= nw * 64) return false;
            const uint64_t x = peek64();
            if (x) {
                const int z = __builtin_clzll(x);
                if (pos + (uint64_t)z >= nw * 64) return false;
                n += (uint64_t)z;
                pos += (uint64_t)z + 1;
                return true;
            }
            n += 64;
            pos += 64;
        }
    }
};

int ilog2(uint64_t x) { return 63 - __builtin_clzll(x); }

bool rice_decode(const std::vector<uint64_t> &w, uint64_t n, uint64_t param, std::vector<uint64_t> &out) {
    if (param > 63) return false;
    BitReader br(w.data(), w.size());
    out.resize(n);
    for (uint64_t i = 0; i < n; i++) {
        uint64_t q, r = 0;
        if (!br.unary(q) || (param && !br.get((int)param, r))) return false;
        out[i] = (q << param) | r;
    }
    return true;
}

bool minimal_binary_decode(const std::vector<uint64_t> &w, uint64_t n, uint64_t param, std::vector<uint64_t> &out) {
    if (param < 1) return n == 0;
    BitReader br(w.data(), w.size());
    const int l = ilog2(param);
    const uint64_t limit = (l == 63 ? 0 : (2ULL << l)) - param;
    out.resize(n);
    for (uint64_t i = 0; i < n; i++) {
        uint64_t v;
        if (!br.get(l, v)) return false;
        if (v >= limit) {
            int b;
            if (!br.bit(b)) return false;
            v = ((v << 1) | (uint64_t)b) - limit;
        }
        if (v == 0) return false;
        out[i] = v - 1;
    }
    return true;
}

// ---- deflate engines -------------------------------------------------------------------
bool zlib_deflate(const uint8_t *data, size_t n, std::vector<uint8_t> &out, size_t at) {
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    const size_t bound = deflateBound(&zs, (uLong)n) + 16;
    out.resize(at + bound);
    zs.next_in = const_cast<Bytef *>(data);
    zs.avail_in = (uInt)n;
    zs.next_out = out.data() + at;
    zs.avail_out = (uInt)bound;
    const int rc = deflate(&zs, Z_FINISH);
    const size_t produced = bound - zs.avail_out;
    deflateEnd(&zs);
    if (rc != Z_STREAM_END) return false;
    out.resize(at + produced);
    return true;
}

// libdeflate.so.0 (dlopen; the image ships the runtime library without headers).  One
// compressor per thread: libdeflate compressors are not thread-safe.
struct LibDeflate {
    void *(*alloc_c)(int) = nullptr;
    void (*free_c)(void *) = nullptr;
    size_t (*deflate_c)(void *, const void *, size_t, void *, size_t) = nullptr;
    size_t (*bound_c)(void *, size_t) = nullptr;
    uint32_t (*crc32_c)(uint32_t, const void *, size_t) = nullptr;  // libdeflate_crc32 (optional)
    bool ok = false;
    LibDeflate() {
        void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc_c = (void *(*)(int))dlsym(h, "libdeflate_alloc_compressor");
        free_c = (void (*)(void *))dlsym(h, "libdeflate_free_compressor");
        deflate_c = (size_t(*)(void *, const void *, size_t, void *, size_t))dlsym(h, "libdeflate_deflate_compress");
        bound_c = (size_t(*)(void *, size_t))dlsym(h, "libdeflate_deflate_compress_bound");
        crc32_c = (uint32_t(*)(uint32_t, const void *, size_t))dlsym(h, "libdeflate_crc32");
        ok = alloc_c && free_c && deflate_c && bound_c;
    }
};
LibDeflate &libdeflate() {
    static LibDeflate L;
    return L;
}
struct ThreadCompressor {
    void *c = nullptr;
    ~ThreadCompressor() {
        if (c) libdeflate().free_c(c);
    }
};
thread_local ThreadCompressor tl_compressor;

bool libdeflate_deflate(const uint8_t *data, size_t n, std::vector<uint8_t> &out, size_t at) {
    LibDeflate &L = libdeflate();
    if (!L.ok) return false;
    if (!tl_compressor.c && !(tl_compressor.c = L.alloc_c(6))) return false;
    const size_t bound = L.bound_c(tl_compressor.c, n);
    out.resize(at + bound);
    const size_t got = L.deflate_c(tl_compressor.c, data, n, out.data() + at, bound);
    if (!got && n) return false;
    out.resize(at + got);
    return true;
}

// order-0 entropy of p[0, n) in bits per byte
double entropy0(const uint8_t *p, size_t n) {
    if (!n) return 0;
    uint32_t h[4][256] = {};
    size_t i = 0;
    for (; i + 4 <= n; i += 4) h[0][p[i]]++, h[1][p[i + 1]]++, h[2][p[i + 2]]++, h[3][p[i + 3]]++;
    for (; i < n; i++) h[0][p[i]]++;
    double e = 0;
    for (int c = 0; c < 256; c++) {
        const uint32_t k = h[0][c] + h[1][c] + h[2][c] + h[3][c];
        if (k) e -= (double)k * std::log2((double)k / (double)n);
    }
    return e / (double)n;
}

// raw deflate of stored blocks (BTYPE 00, at most 65,535 bytes each; one empty final block
// for n = 0), appended to out
void stored_deflate(const uint8_t *data, size_t n, std::vector<uint8_t> &out) {
    size_t i = 0;
    do {
        const size_t len = std::min<size_t>(n - i, 65535);
        const bool last = i + len == n;
        const uint8_t h[5] = {(uint8_t)(last ? 1 : 0), (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)~len,
                              (uint8_t)(~len >> 8)};
        out.insert(out.end(), h, h + 5);
        out.insert(out.end(), data + i, data + i + len);
        i += len;
    } while (i < n);
}

constexpr size_t kEntropySample = 32u << 10;
constexpr double kStoreEntropy = 7.9;

// one gzip member (flate2 GzEncoder shape) appended to out
bool gzip_append(const uint8_t *data, size_t n, int engine, std::vector<uint8_t> &out) {
    static const uint8_t hdr[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    const size_t start = out.size();
    if (engine == NTC_DEFLATE_GPU) {  // the device coder's host restatement (deflate_core.h): the same bytes
        out.resize(start + ntc::df_member_bound(n));
        out.resize(start + ntc::df_member_host(data, n, out.data() + start));
        return true;
    }
    out.insert(out.end(), hdr, hdr + 10);
    bool ok = true;
    if (engine == NTC_DEFLATE_ADAPTIVE && n >= 4096 && entropy0(data, std::min(n, kEntropySample)) >= kStoreEntropy)
        stored_deflate(data, n, out);
    else if (engine == NTC_DEFLATE_LIBDEFLATE || engine == NTC_DEFLATE_ADAPTIVE)
        ok = libdeflate_deflate(data, n, out, start + 10);
    else
        ok = zlib_deflate(data, n, out, start + 10);
    if (!ok) return false;
    LibDeflate &L = libdeflate();  // the same CRC-32 either way; libdeflate's is ~10x faster
    const uint32_t crc = L.ok && L.crc32_c ? L.crc32_c(0, data, n) : (uint32_t)crc32(0L, data, (uInt)n),
                   isize = (uint32_t)n;
    for (int i = 0; i < 4; i++) out.push_back((uint8_t)(crc >> (8 * i)));
    for (int i = 0; i < 4; i++) out.push_back((uint8_t)(isize >> (8 * i)));
    return true;
}

// libdeflate gzip inflate (one decompressor per thread) into a buffer of the expected size
struct LibInflate {
    void *(*alloc_d)() = nullptr;
    void (*free_d)(void *) = nullptr;
    int (*gz_d)(void *, const void *, size_t, void *, size_t, size_t *) = nullptr;
    bool ok = false;
    LibInflate() {
        void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc_d = (void *(*)())dlsym(h, "libdeflate_alloc_decompressor");
        free_d = (void (*)(void *))dlsym(h, "libdeflate_free_decompressor");
        gz_d = (int (*)(void *, const void *, size_t, void *, size_t, size_t *))dlsym(h, "libdeflate_gzip_decompress");
        ok = alloc_d && free_d && gz_d;
    }
};
LibInflate &libinflate() {
    static LibInflate L;
    return L;
}
struct ThreadDecompressor {
    void *d = nullptr;
    ~ThreadDecompressor() {
        if (d) libinflate().free_d(d);
    }
};
thread_local ThreadDecompressor tl_decompressor;

// exactly `want` bytes out of one gzip member, or false (libdeflate when present, else zlib)
bool gunzip_exact(const uint8_t *data, size_t n, size_t want, std::vector<uint8_t> &out);

bool gunzip_bytes(const uint8_t *data, size_t n, std::vector<uint8_t> &out) {
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, 15 + 16) != Z_OK) return false;
    out.clear();
    zs.next_in = const_cast<Bytef *>(data);
    zs.avail_in = (uInt)n;
    uint8_t buf[1 << 16];
    int rc;
    do {
        zs.next_out = buf;
        zs.avail_out = sizeof(buf);
        rc = inflate(&zs, Z_NO_FLUSH);
        if (rc != Z_OK && rc != Z_STREAM_END) {
            inflateEnd(&zs);
            return false;
        }
        out.insert(out.end(), buf, buf + (sizeof(buf) - zs.avail_out));
    } while (rc != Z_STREAM_END);
    inflateEnd(&zs);
    return true;
}

// ---- block header: bincode fixed-int little-endian, 32 bytes (lib.rs:37-50) ------------
struct BlockHeader {
    uint32_t block_size, num_records, num_u64, encoded_size;
    uint64_t rice_param;
    uint8_t bitpacker_exponent, placeholder1;
    uint32_t placeholder2;
    uint16_t placeholder3;
};

void put_le(std::vector<uint8_t> &o, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; i++) o.push_back((uint8_t)(v >> (8 * i)));
}
uint64_t get_le(const uint8_t *p, int bytes) {
    uint64_t v = 0;
    for (int i = 0; i < bytes; i++) v |= (uint64_t)p[i] << (8 * i);
    return v;
}
void write_header(std::vector<uint8_t> &o, const BlockHeader &h) {
    put_le(o, h.block_size, 4);
    put_le(o, h.num_records, 4);
    put_le(o, h.num_u64, 4);
    put_le(o, h.encoded_size, 4);
    put_le(o, h.rice_param, 8);
    put_le(o, h.bitpacker_exponent, 1);
    put_le(o, h.placeholder1, 1);
    put_le(o, h.placeholder2, 4);
    put_le(o, h.placeholder3, 2);
}
BlockHeader read_header(const uint8_t *p) {
    BlockHeader h;
    h.block_size = (uint32_t)get_le(p, 4);
    h.num_records = (uint32_t)get_le(p + 4, 4);
    h.num_u64 = (uint32_t)get_le(p + 8, 4);
    h.encoded_size = (uint32_t)get_le(p + 12, 4);
    h.rice_param = get_le(p + 16, 8);
    h.bitpacker_exponent = p[24];
    h.placeholder1 = p[25];
    h.placeholder2 = (uint32_t)get_le(p + 26, 4);
    h.placeholder3 = (uint16_t)get_le(p + 30, 2);
    return h;
}

inline uint64_t bswap64(uint64_t x) { return __builtin_bswap64(x); }

bool gunzip_exact(const uint8_t *data, size_t n, size_t want, std::vector<uint8_t> &out) {
    LibInflate &L = libinflate();
    if (L.ok && (tl_decompressor.d || (tl_decompressor.d = L.alloc_d()))) {
        out.resize(want);
        size_t got = 0;
        // libdeflate needs the whole member; a longer (corrupt) one fails with short output
        if (L.gz_d(tl_decompressor.d, data, n, out.data(), want, &got) == 0) return got == want;
        return false;
    }
    if (!gunzip_bytes(data, n, out)) return false;
    return out.size() == want;
}

bool decompress_block(const uint8_t *payload, const BlockHeader &h, bool rice, std::vector<uint64_t> &out) {
    std::vector<uint8_t> bytes;
    if (!gunzip_exact(payload, h.block_size, (size_t)h.encoded_size * 8, bytes)) return false;
    std::vector<uint64_t> words(bytes.size() / 8);
    for (size_t i = 0; i < words.size(); i++) {  // big-endian words (see pack_block)
        uint64_t w;
        std::memcpy(&w, bytes.data() + 8 * i, 8);
        words[i] = bswap64(w);
    }
    if (words.size() != h.encoded_size) return false;  // decode.rs:90-92
    return rice ? rice_decode(words, h.num_u64, h.rice_param, out)
                : minimal_binary_decode(words, h.num_u64, h.rice_param, out);
}

// Rice code length of v with parameter p
inline uint64_t rice_bits(uint64_t v, int p) { return (v >> p) + 1 + (uint64_t)p; }

}  // namespace

extern "C" {

void ntc_file_header(uint8_t out[32]) { std::memset(out, 0, 32); }

// split_encoded_dictionary (encode.rs:168-229) + rice / minimal binary coding
// (encode.rs:59-94), words written as compress_block hands them to deflate.
int ntc_pack_block(const uint64_t *recs, uint64_t n_recs, uint64_t num_records, ntc_block_meta *meta,
                   uint8_t **payload, uint64_t *payload_len) {
    if (!meta || !payload || !payload_len || (n_recs && !recs)) return NTC_ERR_INVALID_ARG;
    *payload = nullptr;
    *payload_len = 0;
    std::memset(meta, 0, sizeof(*meta));
    meta->num_records = num_records;
    meta->n_recs = n_recs;
    if (n_recs == 0) return meta->status = NTC_ERR_EMPTY_READ;  // split_encoded_dictionary EncodeError
    // pass 1: stream totals
    uint64_t n_long = 0, max1 = 0, sum2 = 0, sum3 = 0, T = 0;
    for (uint64_t i = 0; i < n_recs; i++) {
        const uint64_t w = recs[i], flag = w >> 56;
        sum3 += flag;
        if ((flag & 2) == 0) {
            n_long++;
            const uint64_t c = w & 0xFFFFFFFFULL;
            max1 = c > max1 ? c : max1;
            sum2 += (w >> 32) & 0xFFFFFFULL;
        } else {
            T += flag >> 2;
        }
    }
    // s4 chunk values: the short bases in 31-base as_2bit chunks.  A short record's bases
    // are bits 0-55 (encode.rs:216-221: from_2bit of bytes 0..7); from_2bit panics past 32
    // bases, so a longer length is a malformed block here.
    std::vector<uint64_t> s4((T + 30) / 31);
    uint64_t max4 = 0;
    {
        uint64_t chunk = 0, nchunk = 0;
        int have = 0;  // bases in chunk
        for (uint64_t i = 0; i < n_recs; i++) {
            const uint64_t w = recs[i], flag = w >> 56;
            if ((flag & 2) == 0) continue;
            int len = (int)(flag >> 2);
            if (len > 32) return meta->status = NTC_ERR_FORMAT;
            uint64_t bits = w & 0x00FFFFFFFFFFFFFFULL;
            if (len < 28) bits &= (1ULL << (2 * len)) - 1;
            while (len) {
                const int take = len < 31 - have ? len : 31 - have;  // <= 31
                chunk |= (bits & ((1ULL << (2 * take)) - 1)) << (2 * have);
                bits >>= 2 * take;
                have += take;
                len -= take;
                if (have == 31) {
                    s4[nchunk++] = chunk;
                    max4 = chunk > max4 ? chunk : max4;
                    chunk = 0;
                    have = 0;
                }
            }
        }
        if (have) {
            s4[nchunk++] = chunk;
            max4 = chunk > max4 ? chunk : max4;
        }
    }
    // write_block_to computes all four before writing: an empty minimal-binary stream errs
    // and the block is dropped (lib.rs:242-250, App. B.3)
    if (n_long == 0 || T == 0) return meta->status = NTC_ERR_EMPTY_READ;
    const int p2 = ntc_rice_log2_b(n_long, sum2), p3 = ntc_rice_log2_b(n_recs, sum3);
    const uint64_t m1 = max1 + 2, m4 = max4 + 2;
    const int l1 = ilog2(m1), l4 = ilog2(m4);
    const uint64_t lim1 = (2ULL << l1) - m1, lim4 = (l4 == 63 ? 0 : (2ULL << l4)) - m4;
    // pass 2: exact code lengths
    uint64_t b1 = 0, b2 = 0, b3 = 0, b4 = 0;
    for (uint64_t i = 0; i < n_recs; i++) {
        const uint64_t w = recs[i], flag = w >> 56;
        b3 += rice_bits(flag, p3);
        if ((flag & 2) == 0) {
            b1 += (uint64_t)l1 + ((w & 0xFFFFFFFFULL) + 1 >= lim1);
            b2 += rice_bits((w >> 32) & 0xFFFFFFULL, p2);
        }
    }
    for (uint64_t v : s4) b4 += (uint64_t)l4 + (v + 1 >= lim4);
    const uint64_t wn[4] = {(b1 + 63) / 64, (b2 + 63) / 64, (b3 + 63) / 64, (b4 + 63) / 64};
    const uint64_t total_words = wn[0] + wn[1] + wn[2] + wn[3];
    uint64_t *words = (uint64_t *)std::malloc(total_words * 8 + 8);
    if (!words) return NTC_ERR_CAPACITY;
    uint64_t off = 0;
    const uint64_t params[4] = {m1, (uint64_t)p2, (uint64_t)p3, m4};
    const uint64_t counts[4] = {n_long, n_long, n_recs, (uint64_t)s4.size()};
    for (int s = 0; s < 4; s++) {
        meta->stream[s].num_u64 = counts[s];
        meta->stream[s].encoded_size = wn[s];
        meta->stream[s].param = params[s];
        meta->stream[s].offset = off * 8;
        off += wn[s];
    }
    // pass 3: codes
    BitSink o1(words), o2(words + wn[0]), o3(words + wn[0] + wn[1]), o4(words + wn[0] + wn[1] + wn[2]);
    const uint64_t mask2 = (1ULL << p2) - 1, mask3 = (1ULL << p3) - 1;
    for (uint64_t i = 0; i < n_recs; i++) {
        const uint64_t w = recs[i], flag = w >> 56;
        o3.zeros(flag >> p3);
        o3.put(((uint64_t)1 << p3) | (flag & mask3), p3 + 1);
        if ((flag & 2) == 0) {
            const uint64_t v = (w & 0xFFFFFFFFULL) + 1;
            if (v < lim1) o1.put(v, l1);
            else o1.put(v + lim1, l1 + 1);
            const uint64_t len = (w >> 32) & 0xFFFFFFULL;
            o2.zeros(len >> p2);
            o2.put(((uint64_t)1 << p2) | (len & mask2), p2 + 1);
        }
    }
    for (uint64_t c : s4) {
        const uint64_t v = c + 1;
        if (v < lim4) o4.put(v, l4);
        else o4.put(v + lim4, l4 + 1);  // v + lim4 < 2^(l4+1) <= 2^63: fits
    }
    const uint64_t got[4] = {o1.finish(), o2.finish(), o3.finish(), o4.finish()};
    for (int s = 0; s < 4; s++)
        if (got[s] != wn[s]) {
            std::free(words);
            return NTC_ERR_FORMAT;  // internal size mismatch (never expected)
        }
    for (uint64_t i = 0; i < total_words; i++) words[i] = bswap64(words[i]);  // on-disk byte order
    *payload = (uint8_t *)words;
    *payload_len = total_words * 8;
    return meta->status = NTC_OK;
}

// compress_block's header + deflate_bytes for each stream (encode.rs:96-127)
}  // extern "C"

namespace {
// stream s of a block: its 32-byte header (write_block_to's fields) + gzip member, appended
int deflate_stream_into(const ntc_block_meta *meta, int s, const uint8_t *payload, int engine,
                        std::vector<uint8_t> &buf) {
    const ntc_stream_meta &m = meta->stream[s];
    const size_t hpos = buf.size();
    buf.resize(hpos + 32);
    if (!gzip_append(payload + m.offset, m.encoded_size * 8, engine, buf)) return NTC_ERR_FORMAT;
    ntc::stream_header(buf.data() + hpos, *meta, s, buf.size() - hpos - 32);
    return NTC_OK;
}

}  // namespace

void ntc::stream_header(uint8_t out[32], const ntc_block_meta &meta, int s, uint64_t member_bytes) {
    const ntc_stream_meta &m = meta.stream[s];
    BlockHeader h{};
    h.block_size = (uint32_t)member_bytes;
    h.num_records = (uint32_t)meta.num_records;
    h.num_u64 = (uint32_t)m.num_u64;
    h.encoded_size = (uint32_t)m.encoded_size;
    h.rice_param = m.param;
    h.bitpacker_exponent = 8;
    std::vector<uint8_t> hb;
    write_header(hb, h);
    std::memcpy(out, hb.data(), 32);
}
bool ntc::libdeflate_loaded() { return libdeflate().ok; }

namespace {
int deflate_checks(const ntc_block_meta *meta, const uint8_t *payload, int engine, uint8_t **out, uint64_t *out_len) {
    if (!meta || !out || !out_len) return NTC_ERR_INVALID_ARG;
    *out = nullptr;
    *out_len = 0;
    if (meta->status != NTC_OK) return meta->status;
    if (!payload) return NTC_ERR_INVALID_ARG;
    if (engine != NTC_DEFLATE_ZLIB && engine != NTC_DEFLATE_LIBDEFLATE && engine != NTC_DEFLATE_ADAPTIVE &&
        engine != NTC_DEFLATE_GPU)
        return NTC_ERR_INVALID_ARG;
    if (engine != NTC_DEFLATE_ZLIB && engine != NTC_DEFLATE_GPU && !libdeflate().ok) return NTC_ERR_UNSUPPORTED;
    return NTC_OK;
}

// the side sections take the host engines only (NTC_DEFLATE_GPU codes block streams)
bool side_engine_ok(int engine) {
    return engine == NTC_DEFLATE_ZLIB || engine == NTC_DEFLATE_LIBDEFLATE || engine == NTC_DEFLATE_ADAPTIVE;
}

int hand_out(const std::vector<uint8_t> &buf, uint8_t **out, uint64_t *out_len) {
    uint8_t *o = (uint8_t *)std::malloc(buf.size() ? buf.size() : 1);
    if (!o) return NTC_ERR_CAPACITY;
    std::memcpy(o, buf.data(), buf.size());
    *out = o;
    *out_len = buf.size();
    return NTC_OK;
}

// ---- what the side-file readers share (ntc_nx_read, ntc_q_read, ntc_n_read, ntc_d_read) ----
// the whole file into buf
int slurp(const char *path, std::vector<uint8_t> &buf) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return NTC_ERR_IO;
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    const bool io_bad = std::ferror(f) != 0;
    std::fclose(f);
    return io_bad ? NTC_ERR_IO : NTC_OK;
}
// The 32-byte header of a side file: the tag, a version 1..max_version and three zero bytes;
// bytes [8, zero_from) are the file's own fields, the rest must be zero.
bool side_header(const std::vector<uint8_t> &buf, const char *tag, uint32_t max_version, size_t zero_from) {
    if (buf.size() < 32 || std::memcmp(buf.data(), tag, 4) != 0) return false;
    if (buf[4] < 1 || buf[4] > max_version || buf[5] || buf[6] || buf[7]) return false;
    for (size_t i = zero_from; i < 32; i++)
        if (buf[i]) return false;
    return true;
}
// a vector handed to the caller as a malloc'd array (ntc_buffer_free); an empty one as null
template <class T>
int hand_out_array(const std::vector<T> &v, T **out) {
    *out = nullptr;
    if (v.empty()) return NTC_OK;
    *out = (T *)std::malloc(v.size() * sizeof(T));
    if (!*out) return NTC_ERR_CAPACITY;
    std::memcpy(*out, v.data(), v.size() * sizeof(T));
    return NTC_OK;
}
// the sections of a file and their payload, both or neither
template <class Meta>
int hand_out_sections(const std::vector<Meta> &all, const std::vector<uint8_t> &pay, Meta **metas, uint64_t *n_blocks,
                      uint8_t **payload, uint64_t *payload_bytes) {
    int rc = hand_out_array(all, metas);
    if (rc) return rc;
    if ((rc = hand_out_array(pay, payload))) {
        std::free(*metas);
        *metas = nullptr;
        return rc;
    }
    *n_blocks = all.size();
    *payload_bytes = pay.size();
    return NTC_OK;
}
// work(i, scratch) for every member i < n, side by side on up to 16 threads (a file of whole
// blocks holds ~10 MB each); false once one of them fails
template <class Work>
bool inflate_members(size_t n, const Work &work) {
    std::atomic<size_t> next{0};
    std::atomic<bool> bad{false};
    const auto run = [&] {
        std::vector<uint8_t> scratch;
        for (size_t i; (i = next.fetch_add(1)) < n && !bad;)
            if (!work(i, scratch)) bad = true;
    };
    const size_t T = std::min<size_t>(n, (size_t)std::max(1, std::min(16, ntc_host_threads())));
    std::vector<std::thread> pool;
    for (size_t t = 1; t < T; t++) pool.emplace_back(run);
    run();
    for (auto &t : pool) t.join();
    return !bad;
}
}  // namespace

extern "C" {

int ntc_deflate_block(const ntc_block_meta *meta, const uint8_t *payload, int engine, uint8_t **out,
                      uint64_t *out_len) {
    int rc = deflate_checks(meta, payload, engine, out, out_len);
    if (rc) return rc;
    std::vector<uint8_t> buf;
    uint64_t est = 0;
    for (int s = 0; s < 4; s++) est += meta->stream[s].encoded_size * 8 + 64;
    buf.reserve(est + est / 16);
    for (int s = 0; s < 4; s++)
        if ((rc = deflate_stream_into(meta, s, payload, engine, buf))) return rc;
    return hand_out(buf, out, out_len);
}

int ntc_deflate_stream(const ntc_block_meta *meta, int stream, const uint8_t *payload, int engine, uint8_t **out,
                       uint64_t *out_len) {
    if (stream < 0 || stream > 3) return NTC_ERR_INVALID_ARG;
    int rc = deflate_checks(meta, payload, engine, out, out_len);
    if (rc) return rc;
    std::vector<uint8_t> buf;
    buf.reserve(meta->stream[stream].encoded_size * 8 + meta->stream[stream].encoded_size / 2 + 128);
    if ((rc = deflate_stream_into(meta, stream, payload, engine, buf))) return rc;
    return hand_out(buf, out, out_len);
}

int ntc_write_block(const uint64_t *recs, uint64_t n_recs, uint64_t num_records, uint8_t **out, uint64_t *out_len) {
    if (!out || !out_len || (n_recs && !recs)) return NTC_ERR_INVALID_ARG;
    *out = nullptr;
    *out_len = 0;
    ntc_block_meta meta;
    uint8_t *payload = nullptr;
    uint64_t plen = 0;
    int rc = ntc_pack_block(recs, n_recs, num_records, &meta, &payload, &plen);
    if (rc == NTC_OK) rc = ntc_deflate_block(&meta, payload, NTC_DEFLATE_ZLIB, out, out_len);
    std::free(payload);
    return rc;
}

}  // extern "C"

namespace {
// zip_block_contents (decode.rs:102-149): the four decoded streams -> u64 records, into vec
// (resized) or out (cap records; NTC_ERR_CAPACITY if more).  *n_recs = the block's records.
int zip_parts(const std::vector<uint64_t> (&parts)[4], std::vector<uint64_t> *vec, uint64_t *out, uint64_t cap,
              uint64_t *n_recs) {
    const auto &c1 = parts[0], &c2 = parts[1], &fl = parts[2], &bn = parts[3];
    if (c1.size() != c2.size()) return NTC_ERR_FORMAT;
    uint64_t T = 0;
    for (uint64_t f : fl) T += (f & 0xFC) >> 2;
    // short-record bases: chunk i holds 31 bases, the last one the rest.  decode.rs:114-118
    // uses T % 31 for the last chunk, which panics whenever T is a positive multiple of 31
    // (Appendix B.4); ((T-1) % 31) + 1 agrees everywhere else
    if (T ? bn.size() != (T + 30) / 31 : false) return NTC_ERR_FORMAT;
    *n_recs = fl.size();
    if (vec) {
        vec->resize(fl.size());
        out = vec->data();
    } else if (fl.size() > cap) {
        return NTC_ERR_CAPACITY;
    }
    size_t i = 0;
    uint64_t j = 0;  // next short base
    for (size_t r = 0; r < fl.size(); r++) {
        const uint8_t flag = (uint8_t)fl[r];
        uint64_t w;
        if ((flag & 2) == 0) {
            if (i >= c1.size()) return NTC_ERR_FORMAT;
            w = (c1[i] & 0xFFFFFFFFULL) | ((c2[i] & 0xFFFFFFULL) << 32);
            i++;
        } else {
            const uint32_t l = flag >> 2;
            if (j + l > T) return NTC_ERR_FORMAT;
            // bases j .. j + l - 1 of the concatenation: from chunk j / 31 (and the next)
            // (past 32 bases the reference's as_2bit panics; here base t lands on bit 2 t mod 64,
            // as in unpack.hip, so the two decoders agree on such a block too)
            w = 0;
            for (uint32_t t = 0; t < l; t++) {
                const uint64_t q = j + t;
                w |= ((bn[q / 31] >> (2 * (q % 31))) & 3ULL) << ((2 * t) & 63);
            }
            w &= 0x00FFFFFFFFFFFFFFULL;
            j += l;
        }
        out[r] = w | ((uint64_t)flag << 56);
    }
    return NTC_OK;
}

// decode_block's container half (lib.rs:320-363): the block's four streams, decompressed and
// zipped back into u64 records (zip_block_contents, decode.rs:102-149), into vec (resized)
// or out (cap records; NTC_ERR_CAPACITY if more).  *n_recs = the block's record count.
int read_block_impl(const uint8_t *data, uint64_t len, uint64_t *consumed, std::vector<uint64_t> *vec, uint64_t *out,
                    uint64_t cap, uint64_t *n_recs, uint64_t *num_records) {
    *n_recs = 0;
    *consumed = 0;
    uint64_t pos = 0;
    std::vector<uint64_t> parts[4];
    BlockHeader hs[4];
    for (int s = 0; s < 4; s++) {
        if (pos + 32 > len) return s == 0 && pos == len ? NTC_ERR_IO : NTC_ERR_FORMAT;  // IO = clean EOF
        hs[s] = read_header(data + pos);
        pos += 32;
        if (pos + hs[s].block_size > len) return NTC_ERR_FORMAT;
        if (!decompress_block(data + pos, hs[s], s == 1 || s == 2, parts[s])) return NTC_ERR_FORMAT;
        pos += hs[s].block_size;
    }
    const int rc = zip_parts(parts, vec, out, cap, n_recs);
    if (rc == NTC_OK || rc == NTC_ERR_CAPACITY) {
        *consumed = pos;
        if (num_records) *num_records = hs[0].num_records;
    }
    return rc;
}
}  // namespace

namespace ntc {
// The GPU unpacker's work on the host (the sanitizer builds' stand-in for the device): one
// block's inflated streams (payload at meta's offsets) -> records; NTC_ERR_FORMAT if damaged.
int unpack_block_host(const ntc_block_meta &m, const uint8_t *payload, std::vector<uint64_t> &recs) {
    std::vector<uint64_t> parts[4];
    for (int s = 0; s < 4; s++) {
        const ntc_stream_meta &st = m.stream[s];
        std::vector<uint64_t> words(st.encoded_size);
        for (uint64_t i = 0; i < st.encoded_size; i++) {
            uint64_t w;
            std::memcpy(&w, payload + st.offset + 8 * i, 8);
            words[i] = bswap64(w);
        }
        const bool ok = (s == 1 || s == 2) ? rice_decode(words, st.num_u64, st.param, parts[s])
                                           : minimal_binary_decode(words, st.num_u64, st.param, parts[s]);
        if (!ok) return NTC_ERR_FORMAT;
    }
    uint64_t n = 0;
    return zip_parts(parts, &recs, nullptr, 0, &n);
}
}  // namespace ntc

extern "C" {

int ntc_read_block(const uint8_t *data, uint64_t len, uint64_t *consumed, uint64_t **recs, uint64_t *n_recs,
                   uint64_t *num_records) {
    if (!data || !consumed || !recs || !n_recs) return NTC_ERR_INVALID_ARG;
    *recs = nullptr;
    std::vector<uint64_t> v;
    uint64_t used = 0;
    const int rc = read_block_impl(data, len, &used, &v, nullptr, 0, n_recs, num_records);
    if (rc) {
        *n_recs = 0;
        *consumed = 0;
        return rc;
    }
    uint64_t *buf = (uint64_t *)std::malloc((v.size() ? v.size() : 1) * 8);
    if (!buf) return NTC_ERR_CAPACITY;
    std::memcpy(buf, v.data(), v.size() * 8);
    *recs = buf;
    *consumed = used;
    return NTC_OK;
}

int ntc_read_block_streams(const uint8_t *data, uint64_t len, uint64_t *consumed, uint8_t *payload,
                           uint64_t capacity, ntc_block_meta *meta) {
    if (!data || !consumed || !meta || (capacity && !payload)) return NTC_ERR_INVALID_ARG;
    *consumed = 0;
    std::memset(meta, 0, sizeof(*meta));
    uint64_t pos = 0, off = 0;
    BlockHeader hs[4];
    for (int s = 0; s < 4; s++) {
        if (pos + 32 > len) return s == 0 && pos == len ? NTC_ERR_IO : NTC_ERR_FORMAT;  // IO = clean EOF
        hs[s] = read_header(data + pos);
        pos += 32;
        if (pos + hs[s].block_size > len) return NTC_ERR_FORMAT;
        const uint64_t want = (uint64_t)hs[s].encoded_size * 8;
        if (off + want > capacity) return NTC_ERR_CAPACITY;
        // libdeflate straight into the payload; zlib through a vector
        LibInflate &L = libinflate();
        bool ok = false;
        if (L.ok && (tl_decompressor.d || (tl_decompressor.d = L.alloc_d()))) {
            size_t got = 0;
            ok = L.gz_d(tl_decompressor.d, data + pos, hs[s].block_size, payload + off, want, &got) == 0 && got == want;
        } else {
            std::vector<uint8_t> v;
            ok = gunzip_bytes(data + pos, hs[s].block_size, v) && v.size() == want;
            if (ok && want) std::memcpy(payload + off, v.data(), want);
        }
        if (!ok) return NTC_ERR_FORMAT;
        meta->stream[s].num_u64 = hs[s].num_u64;
        meta->stream[s].encoded_size = hs[s].encoded_size;
        meta->stream[s].param = hs[s].rice_param;
        meta->stream[s].offset = off;
        off += want;
        pos += hs[s].block_size;
    }
    meta->num_records = hs[0].num_records;
    meta->n_recs = hs[2].num_u64;
    *consumed = pos;
    return NTC_OK;
}

int ntc_read_block_into(const uint8_t *data, uint64_t len, uint64_t *consumed, uint64_t *recs, uint64_t capacity,
                        uint64_t *n_recs, uint64_t *num_records) {
    if (!data || !consumed || !n_recs || (capacity && !recs)) return NTC_ERR_INVALID_ARG;
    return read_block_impl(data, len, consumed, nullptr, recs, capacity, n_recs, num_records);
}

void ntc_buffer_free(void *p) { std::free(p); }

// ---- exception side file "NTCX" (include/ntcomp_codec.h) ------------------------------
static_assert(sizeof(ntc_nx_run) == 24, "ntc_nx_run is the file's run record");

static bool nx_write_all(int fd, const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    while (n) {
        const ssize_t w = ::write(fd, b, n);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return false;
        b += w;
        n -= (size_t)w;
    }
    return true;
}

int ntc_nx_write(int fd, const ntc_nx_run *runs, uint64_t n_runs, uint32_t sub, int with_header) {
    if (fd < 0 || (n_runs && !runs) || !ntc::nx_is_base(sub)) return NTC_ERR_INVALID_ARG;
    if (with_header) {
        uint8_t h[32] = {'N', 'T', 'C', 'X', 1, 0, 0, 0, (uint8_t)sub};
        if (!nx_write_all(fd, h, sizeof(h))) return NTC_ERR_IO;
    }
    if (n_runs) {
        const uint64_t sec[2] = {n_runs, 0};  // little-endian hosts only, as the block container
        if (!nx_write_all(fd, sec, sizeof(sec)) || !nx_write_all(fd, runs, n_runs * sizeof(ntc_nx_run))) return NTC_ERR_IO;
    }
    return NTC_OK;
}

int ntc_nx_read(const char *path, ntc_nx_run **runs, uint64_t *n_runs, uint32_t *sub) {
    if (!path || !runs || !n_runs || !sub) return NTC_ERR_INVALID_ARG;
    *runs = nullptr;
    *n_runs = 0;
    *sub = 0;
    std::vector<uint8_t> buf;
    if (const int rc = slurp(path, buf)) return rc;
    if (!side_header(buf, "NTCX", 1, 9) || !ntc::nx_is_base(buf[8])) return NTC_ERR_FORMAT;
    std::vector<ntc_nx_run> all;
    size_t at = 32;
    while (at < buf.size()) {
        uint64_t sec[2];
        if (buf.size() - at < 16) return NTC_ERR_FORMAT;
        std::memcpy(sec, buf.data() + at, 16);
        at += 16;
        if (sec[1] != 0 || sec[0] == 0 || sec[0] > (buf.size() - at) / sizeof(ntc_nx_run)) return NTC_ERR_FORMAT;
        const size_t first = all.size();
        all.resize(first + sec[0]);
        std::memcpy(all.data() + first, buf.data() + at, sec[0] * sizeof(ntc_nx_run));
        at += sec[0] * sizeof(ntc_nx_run);
    }
    for (size_t i = 0; i < all.size(); i++) {
        const ntc_nx_run &r = all[i];
        if (r.len == 0 || r.reserved != 0 || !ntc::nx_is_symbol(r.sym) || (uint64_t)r.pos + r.len > (1ull << 32))
            return NTC_ERR_FORMAT;
        if (i) {  // strictly after the run before it, and clear of it
            const ntc_nx_run &p = all[i - 1];
            if (r.read < p.read || (r.read == p.read && (uint64_t)r.pos < (uint64_t)p.pos + p.len)) return NTC_ERR_FORMAT;
        }
    }
    if (const int rc = hand_out_array(all, runs)) return rc;
    *n_runs = all.size();
    *sub = buf[8];
    return NTC_OK;
}

// ---- quality side file "NTCQ" (include/ntcomp_codec.h) --------------------------------
int ntc_q_write_header(int fd, int mode) {
    if (fd < 0 || mode < 1 || mode > 2) return NTC_ERR_INVALID_ARG;
    const uint8_t h[32] = {'N', 'T', 'C', 'Q', 1, 0, 0, 0, (uint8_t)mode};
    return nx_write_all(fd, h, sizeof(h)) ? NTC_OK : NTC_ERR_IO;
}

int ntc_q_write_header2(int fd, int mode, int coder) {
    if (coder == 0) return ntc_q_write_header(fd, mode);
    if (fd < 0 || mode < 1 || mode > 2 || coder != 1) return NTC_ERR_INVALID_ARG;
    const uint8_t h[32] = {'N', 'T', 'C', 'Q', 2, 0, 0, 0, (uint8_t)mode, (uint8_t)coder};
    return nx_write_all(fd, h, sizeof(h)) ? NTC_OK : NTC_ERR_IO;
}

int ntc_q_deflate_section(const ntc_qual_meta *meta, const uint8_t *words, int engine, uint8_t **out, uint64_t *out_len) {
    if (!meta || !out || !out_len || (meta->payload_bytes && !words)) return NTC_ERR_INVALID_ARG;
    *out = nullptr;
    *out_len = 0;
    if (!side_engine_ok(engine)) return NTC_ERR_INVALID_ARG;
    if (meta->reserved[0] == 1) {  // coder 1: the body as it came off the device, no gzip member
        if (!ntc::q_meta_ok(meta->n_quals, meta->width, meta->n_syms, meta->alphabet) || meta->payload_bytes >> 32 ||
            !ntc::qr_body_ok(meta->n_quals, meta->n_syms, words, meta->payload_bytes))
            return NTC_ERR_INVALID_ARG;
        std::vector<uint8_t> sec(24);
        sec.insert(sec.end(), meta->alphabet, meta->alphabet + meta->n_syms);
        if (meta->payload_bytes) sec.insert(sec.end(), words, words + meta->payload_bytes);
        std::memcpy(sec.data(), &meta->n_reads, 8);
        std::memcpy(sec.data() + 8, &meta->n_quals, 8);
        sec[16] = meta->width;
        sec[17] = meta->n_syms;
        const uint32_t body32 = (uint32_t)meta->payload_bytes;
        std::memcpy(sec.data() + 20, &body32, 4);
        return hand_out(sec, out, out_len);
    }
    if (meta->reserved[0]) return NTC_ERR_INVALID_ARG;
    if (!ntc::q_meta_ok(meta->n_quals, meta->width, meta->n_syms, meta->alphabet) ||
        meta->payload_bytes != ntc::q_words(meta->n_quals, meta->width) * 8)
        return NTC_ERR_INVALID_ARG;
    std::vector<uint8_t> buf(24);
    buf.insert(buf.end(), meta->alphabet, meta->alphabet + meta->n_syms);
    if (meta->width && !gzip_append(words, meta->payload_bytes, engine, buf)) return NTC_ERR_FORMAT;
    const uint64_t gz = buf.size() - 24 - meta->n_syms;
    if (gz >> 32) return NTC_ERR_CAPACITY;
    std::memcpy(buf.data(), &meta->n_reads, 8);  // little-endian hosts only, as the block container
    std::memcpy(buf.data() + 8, &meta->n_quals, 8);
    buf[16] = meta->width;
    buf[17] = meta->n_syms;
    const uint32_t gz32 = (uint32_t)gz;
    std::memcpy(buf.data() + 20, &gz32, 4);
    return hand_out(buf, out, out_len);
}

int ntc_q_write_section(int fd, const ntc_qual_meta *meta, const uint8_t *words, int engine) {
    if (fd < 0) return NTC_ERR_INVALID_ARG;
    uint8_t *sec = nullptr;
    uint64_t n = 0;
    const int rc = ntc_q_deflate_section(meta, words, engine, &sec, &n);
    if (rc) return rc;
    const bool ok = nx_write_all(fd, sec, n);
    std::free(sec);
    return ok ? NTC_OK : NTC_ERR_IO;
}

int ntc_q_read(const char *path, int *mode, ntc_qual_meta **metas, uint64_t *n_blocks, uint8_t **payload,
               uint64_t *payload_bytes) {
    if (!path || !mode || !metas || !n_blocks || !payload || !payload_bytes) return NTC_ERR_INVALID_ARG;
    *mode = 0;
    *metas = nullptr;
    *n_blocks = 0;
    *payload = nullptr;
    *payload_bytes = 0;
    std::vector<uint8_t> buf;
    if (const int rc = slurp(path, buf)) return rc;
    if (!side_header(buf, "NTCQ", 2, 10)) return NTC_ERR_FORMAT;
    const bool v2 = buf[4] == 2;  // version 2: coder 1, the bodies as they are
    if (buf[8] < 1 || buf[8] > 2 || buf[9] != (v2 ? 1 : 0)) return NTC_ERR_FORMAT;
    // pass 1: the headers and alphabets, and where each member lies and inflates to
    std::vector<ntc_qual_meta> all;
    std::vector<uint64_t> gz_at, gz_len;
    uint64_t pay_bytes = 0;
    size_t at = 32;
    while (at < buf.size()) {
        if (buf.size() - at < 24) return NTC_ERR_FORMAT;
        ntc_qual_meta m;
        std::memset(&m, 0, sizeof(m));
        const uint8_t *h = buf.data() + at;
        std::memcpy(&m.n_reads, h, 8);
        std::memcpy(&m.n_quals, h + 8, 8);
        m.width = h[16];
        m.n_syms = h[17];
        uint32_t gz;
        std::memcpy(&gz, h + 20, 4);
        at += 24;
        if (h[18] || h[19] || m.n_syms > 94 || buf.size() - at < m.n_syms) return NTC_ERR_FORMAT;
        std::memcpy(m.alphabet, buf.data() + at, m.n_syms);
        at += m.n_syms;
        if (!ntc::q_meta_ok(m.n_quals, m.width, m.n_syms, m.alphabet) || m.n_quals > m.n_reads * (1ull << 32))
            return NTC_ERR_FORMAT;
        if (buf.size() - at < gz || (gz == 0) != (m.width == 0)) return NTC_ERR_FORMAT;
        if (v2) {  // gz = the body's bytes; every body starts 8-aligned in the payload
            if (!ntc::qr_body_ok(m.n_quals, m.n_syms, buf.data() + at, gz)) return NTC_ERR_FORMAT;
            m.reserved[0] = 1;
            m.payload_off = pay_bytes;
            m.payload_bytes = gz;
            pay_bytes += ((uint64_t)gz + 7) & ~7ull;
            gz_at.push_back(at);
            gz_len.push_back(gz);
            at += gz;
            all.push_back(m);
            continue;
        }
        const uint64_t nw = ntc::q_words(m.n_quals, m.width);
        if (nw * 8 > (uint64_t)gz * 1100 + 4096) return NTC_ERR_FORMAT;  // past deflate's best ratio: not this member
        m.payload_off = pay_bytes;
        m.payload_bytes = nw * 8;
        pay_bytes += nw * 8;
        gz_at.push_back(at);
        gz_len.push_back(gz);
        at += gz;
        all.push_back(m);
    }
    // pass 2: the members inflate side by side
    std::vector<uint8_t> pay(pay_bytes);
    const bool ok = inflate_members(all.size(), [&](size_t i, std::vector<uint8_t> &words) {
        const ntc_qual_meta &m = all[i];
        if (!m.width) return true;
        if (v2) {
            std::memcpy(pay.data() + m.payload_off, buf.data() + gz_at[i], m.payload_bytes);
            return true;
        }
        if (!gunzip_exact(buf.data() + gz_at[i], gz_len[i], m.payload_bytes, words)) return false;
        const uint64_t bits = m.n_quals * m.width;  // padding bits of the last word
        if (bits & 63) {
            uint64_t last;
            std::memcpy(&last, words.data() + m.payload_bytes - 8, 8);
            if (last >> (bits & 63)) return false;
        }
        std::memcpy(pay.data() + m.payload_off, words.data(), m.payload_bytes);
        return true;
    });
    if (!ok) return NTC_ERR_FORMAT;
    if (const int rc = hand_out_sections(all, pay, metas, n_blocks, payload, payload_bytes)) return rc;
    *mode = buf[8];
    return NTC_OK;
}

}  // extern "C"

// ---- name side file "NTCN" (include/ntcomp_codec.h) -----------------------------------
namespace {
// the counts of a meta agree with one another (names_core.h; payload_off is the caller's)
bool n_meta_ok(const ntc_name_meta &m) { return ntc::n_meta_ok(m.n_reads, m.name_bytes, m.mid_bytes, m.payload_bytes); }
// the payload of a section whose meta n_meta_ok took: every per-read rule, the sums, the padding
bool n_section_ok(const ntc_name_meta &m, const uint8_t *p) {
    const uint64_t n = m.n_reads;
    uint64_t names = 0, mids = 0;
    uint32_t plen = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t len = (uint32_t)p[2 * i] | (uint32_t)p[2 * i + 1] << 8, pre = p[2 * n + i], suf = p[3 * n + i];
        if (!ntc::n_read_ok((uint32_t)(i % ntc::kNGroup), len, pre, suf, plen)) return false;
        names += len;
        mids += len - pre - suf;
        plen = len;
    }
    if (names != m.name_bytes || mids != m.mid_bytes) return false;
    for (uint64_t i = 4 * n + mids; i < m.payload_bytes; i++)
        if (p[i]) return false;
    return true;
}
}  // namespace

extern "C" {

int ntc_n_write_header(int fd, int mode) {
    if (fd < 0 || mode < 1 || mode > 2) return NTC_ERR_INVALID_ARG;
    const uint8_t h[32] = {'N', 'T', 'C', 'N', 1, 0, 0, 0, (uint8_t)mode};
    return nx_write_all(fd, h, sizeof(h)) ? NTC_OK : NTC_ERR_IO;
}

int ntc_n_deflate_section(const ntc_name_meta *meta, const uint8_t *payload, int engine, uint8_t **out, uint64_t *out_len) {
    if (!meta || !out || !out_len || (meta->payload_bytes && !payload)) return NTC_ERR_INVALID_ARG;
    *out = nullptr;
    *out_len = 0;
    if (!side_engine_ok(engine)) return NTC_ERR_INVALID_ARG;
    if (!n_meta_ok(*meta) || !n_section_ok(*meta, payload)) return NTC_ERR_INVALID_ARG;
    std::vector<uint8_t> buf(32);
    if (!gzip_append(payload, meta->payload_bytes, engine, buf)) return NTC_ERR_FORMAT;
    const uint64_t gz = buf.size() - 32;
    if (gz >> 32) return NTC_ERR_CAPACITY;
    std::memcpy(buf.data(), &meta->n_reads, 8);  // little-endian hosts only, as the block container
    std::memcpy(buf.data() + 8, &meta->name_bytes, 8);
    std::memcpy(buf.data() + 16, &meta->mid_bytes, 8);
    const uint32_t gz32 = (uint32_t)gz;
    std::memcpy(buf.data() + 24, &gz32, 4);
    return hand_out(buf, out, out_len);
}

int ntc_n_write_section(int fd, const ntc_name_meta *meta, const uint8_t *payload, int engine) {
    if (fd < 0) return NTC_ERR_INVALID_ARG;
    uint8_t *sec = nullptr;
    uint64_t n = 0;
    const int rc = ntc_n_deflate_section(meta, payload, engine, &sec, &n);
    if (rc) return rc;
    const bool ok = nx_write_all(fd, sec, n);
    std::free(sec);
    return ok ? NTC_OK : NTC_ERR_IO;
}

int ntc_n_read(const char *path, int *mode, ntc_name_meta **metas, uint64_t *n_blocks, uint8_t **payload,
               uint64_t *payload_bytes) {
    if (!path || !mode || !metas || !n_blocks || !payload || !payload_bytes) return NTC_ERR_INVALID_ARG;
    *mode = 0;
    *metas = nullptr;
    *n_blocks = 0;
    *payload = nullptr;
    *payload_bytes = 0;
    std::vector<uint8_t> buf;
    if (const int rc = slurp(path, buf)) return rc;
    if (!side_header(buf, "NTCN", 1, 9) || buf[8] < 1 || buf[8] > 2) return NTC_ERR_FORMAT;
    // pass 1: the section headers, and where each member lies and inflates to
    std::vector<ntc_name_meta> all;
    std::vector<uint64_t> gz_at, gz_len;
    uint64_t pay_bytes = 0;
    size_t at = 32;
    while (at < buf.size()) {
        if (buf.size() - at < 32) return NTC_ERR_FORMAT;
        ntc_name_meta m{};
        const uint8_t *h = buf.data() + at;
        std::memcpy(&m.n_reads, h, 8);
        std::memcpy(&m.name_bytes, h + 8, 8);
        std::memcpy(&m.mid_bytes, h + 16, 8);
        uint32_t gz, pad;
        std::memcpy(&gz, h + 24, 4);
        std::memcpy(&pad, h + 28, 4);
        at += 32;
        m.payload_bytes = ntc::n_payload_bytes(m.n_reads & ((1ull << 40) - 1), m.mid_bytes & ((1ull << 48) - 1));
        if (pad || !n_meta_ok(m) || buf.size() - at < gz) return NTC_ERR_FORMAT;
        if (m.payload_bytes > (uint64_t)gz * 1100 + 4096) return NTC_ERR_FORMAT;  // past deflate's best ratio: not this member
        m.payload_off = pay_bytes;
        pay_bytes += m.payload_bytes;
        gz_at.push_back(at);
        gz_len.push_back(gz);
        at += gz;
        all.push_back(m);
    }
    // pass 2: the members inflate and are checked side by side
    std::vector<uint8_t> pay(pay_bytes);
    const bool ok = inflate_members(all.size(), [&](size_t i, std::vector<uint8_t> &sec) {
        const ntc_name_meta &m = all[i];
        if (!gunzip_exact(buf.data() + gz_at[i], gz_len[i], m.payload_bytes, sec) || !n_section_ok(m, sec.data())) return false;
        if (m.payload_bytes) std::memcpy(pay.data() + m.payload_off, sec.data(), m.payload_bytes);
        return true;
    });
    if (!ok) return NTC_ERR_FORMAT;
    if (const int rc = hand_out_sections(all, pay, metas, n_blocks, payload, payload_bytes)) return rc;
    *mode = buf[8];
    return NTC_OK;
}

}  // extern "C"

// ---- digest side file "NTCD" (include/ntcomp_codec.h) ---------------------------------
namespace {
static_assert(sizeof(ntc_digest_meta) == 56, "a section is the meta as it stands");
// a meta on its own (digest_core.h): known bits, seq among them, nothing set for an absent component
bool d_meta_ok(const ntc_digest_meta &m) {
    const uint64_t d[4] = {m.d_seq, m.d_sym, m.d_qual, m.d_name};
    return ntc::dg_meta_ok(m.components, m.reserved, d);
}
}  // namespace

extern "C" {

int ntc_d_write_header(int fd, uint32_t components, uint32_t k, uint64_t n_nodes) {
    if (fd < 0 || (components & ~ntc::kDgAll) || !(components & ntc::kDgSeq)) return NTC_ERR_INVALID_ARG;
    uint8_t h[32] = {'N', 'T', 'C', 'D', 1, 0, 0, 0, (uint8_t)components};
    std::memcpy(h + 12, &k, 4);  // little-endian hosts only, as the block container
    std::memcpy(h + 16, &n_nodes, 8);
    return nx_write_all(fd, h, sizeof(h)) ? NTC_OK : NTC_ERR_IO;
}

int ntc_d_write_section(int fd, const ntc_digest_meta *meta) {
    if (fd < 0 || !meta || !d_meta_ok(*meta)) return NTC_ERR_INVALID_ARG;
    return nx_write_all(fd, (const uint8_t *)meta, sizeof(*meta)) ? NTC_OK : NTC_ERR_IO;
}

int ntc_d_read(const char *path, uint32_t *components, uint32_t *k, uint64_t *n_nodes, ntc_digest_meta **metas,
               uint64_t *n_blocks) {
    if (!path || !components || !k || !n_nodes || !metas || !n_blocks) return NTC_ERR_INVALID_ARG;
    *components = *k = 0;
    *n_nodes = 0;
    *metas = nullptr;
    *n_blocks = 0;
    std::vector<uint8_t> buf;
    if (const int rc = slurp(path, buf)) return rc;
    if (!side_header(buf, "NTCD", 1, 24) || buf[9] || buf[10] || buf[11]) return NTC_ERR_FORMAT;  // (k and n_nodes between)
    const uint32_t comp = buf[8];
    if ((comp & ~ntc::kDgAll) || !(comp & ntc::kDgSeq)) return NTC_ERR_FORMAT;
    if ((buf.size() - 32) % sizeof(ntc_digest_meta)) return NTC_ERR_FORMAT;
    const uint64_t n = (buf.size() - 32) / sizeof(ntc_digest_meta);
    std::vector<ntc_digest_meta> all(n);
    if (n) std::memcpy(all.data(), buf.data() + 32, n * sizeof(ntc_digest_meta));
    for (const ntc_digest_meta &m : all)
        if (!d_meta_ok(m) || (m.components & ~comp)) return NTC_ERR_FORMAT;
    if (const int rc = hand_out_array(all, metas)) return rc;
    std::memcpy(k, buf.data() + 12, 4);
    std::memcpy(n_nodes, buf.data() + 16, 8);
    *components = comp;
    *n_blocks = n;
    return NTC_OK;
}

}  // extern "C"
