// image_io.cpp — float image output/input without tinyexr / stb (absent submodules).
// save_image mirrors src/util/imageio.cpp:694-726: float RGBA -> ".exr" (fp32 channels) or
// ".hdr" (Radiance RGBE); any other extension falls back to ".exr".  The EXR writer emits
// uncompressed scanlines (tinyexr would ZIP them; every OpenEXR reader accepts both).
// Readers: PFM, Radiance HDR, uncompressed scanline EXR (float/half), binary PPM/PGM.
#include "scene.h"

#include <cmath>
#include <cstring>
#include <filesystem>
#include <zlib.h>
#include <fstream>

namespace lr {

namespace fs = std::filesystem;

namespace {

std::string lower_ext(const fs::path &p) {
    auto ext = p.extension().string();
    for (auto &c : ext) { c = static_cast<char>(std::tolower(c)); }
    return ext;
}

template<typename T>
void put(std::string &buf, T v) { buf.append(reinterpret_cast<const char *>(&v), sizeof(T)); }
void put_str(std::string &buf, const char *s) { buf.append(s, std::strlen(s) + 1u); }

// `nc` interleaved channels per pixel: 4 = RGBA, 3 = RGB, 1 = one value.  The channel list is alphabetical and the scanlines follow it:
// A B G R, B G R, or a lone A -- what tinyexr's SaveEXR writes for 4, 3 and 1 components (from memory of tinyexr, which is not part of
// the reference snapshot: it names a single component "A"), all FLOAT here
void write_exr(const fs::path &path, const float *rgba, uint32_t w, uint32_t h, uint32_t nc = 4u) {
    static constexpr const char *kNames4[4] = {"A", "B", "G", "R"}, *kNames3[3] = {"B", "G", "R"}, *kNames1[1] = {"A"};
    static constexpr int kOrder4[4] = {3, 2, 1, 0}, kOrder3[3] = {2, 1, 0}, kOrder1[1] = {0};// source channel of each stored one
    const auto names = nc == 4u ? kNames4 : nc == 3u ? kNames3 : kNames1;
    const auto order = nc == 4u ? kOrder4 : nc == 3u ? kOrder3 : kOrder1;
    std::string head;
    put<uint32_t>(head, 20000630u);// magic
    put<uint32_t>(head, 2u);       // version 2, scanline, single part
    // channels (alphabetical), all FLOAT (pixel type 2)
    put_str(head, "channels"), put_str(head, "chlist");
    put<uint32_t>(head, nc * 18u + 1u);
    for (uint32_t k = 0u; k < nc; k++) {
        const auto name = names[k];
        put_str(head, name);
        put<uint32_t>(head, 2u);// FLOAT
        put<uint8_t>(head, 0u); // pLinear
        head.append(3u, '\0');
        put<uint32_t>(head, 1u), put<uint32_t>(head, 1u);
    }
    put<uint8_t>(head, 0u);
    put_str(head, "compression"), put_str(head, "compression"), put<uint32_t>(head, 1u), put<uint8_t>(head, 0u);
    auto box = [&](const char *name) {
        put_str(head, name), put_str(head, "box2i"), put<uint32_t>(head, 16u);
        put<int32_t>(head, 0), put<int32_t>(head, 0);
        put<int32_t>(head, static_cast<int32_t>(w) - 1), put<int32_t>(head, static_cast<int32_t>(h) - 1);
    };
    box("dataWindow"), box("displayWindow");
    put_str(head, "lineOrder"), put_str(head, "lineOrder"), put<uint32_t>(head, 1u), put<uint8_t>(head, 0u);
    put_str(head, "pixelAspectRatio"), put_str(head, "float"), put<uint32_t>(head, 4u), put<float>(head, 1.f);
    put_str(head, "screenWindowCenter"), put_str(head, "v2f"), put<uint32_t>(head, 8u), put<float>(head, 0.f), put<float>(head, 0.f);
    put_str(head, "screenWindowWidth"), put_str(head, "float"), put<uint32_t>(head, 4u), put<float>(head, 1.f);
    put<uint8_t>(head, 0u);// end of header

    auto line_bytes = static_cast<uint64_t>(w) * 4u * nc;
    auto table_offset = head.size();
    auto data_offset = table_offset + static_cast<uint64_t>(h) * 8u;
    std::ofstream f{path, std::ios::binary};
    if (!f) { throw Error{"Failed to save film to '" + path.string() + "'."}; }
    f.write(head.data(), static_cast<std::streamsize>(head.size()));
    for (uint32_t y = 0; y < h; y++) {
        auto off = data_offset + static_cast<uint64_t>(y) * (8u + line_bytes);
        f.write(reinterpret_cast<const char *>(&off), 8);
    }
    std::vector<float> line(static_cast<size_t>(w) * nc);
    for (uint32_t y = 0; y < h; y++) {
        auto yy = static_cast<int32_t>(y);
        auto size = static_cast<uint32_t>(line_bytes);
        f.write(reinterpret_cast<const char *>(&yy), 4);
        f.write(reinterpret_cast<const char *>(&size), 4);
        for (uint32_t c = 0u; c < nc; c++) {
            for (uint32_t x = 0; x < w; x++) {
                line[static_cast<size_t>(c) * w + x] = rgba[(static_cast<size_t>(y) * w + x) * nc + static_cast<size_t>(order[c])];
            }
        }
        f.write(reinterpret_cast<const char *>(line.data()), static_cast<std::streamsize>(line_bytes));
    }
}

void float_to_rgbe(const float *rgb, uint8_t *out) {
    auto m = std::max(rgb[0], std::max(rgb[1], rgb[2]));
    if (m < 1e-32f) {
        out[0] = out[1] = out[2] = out[3] = 0u;
        return;
    }
    int e;
    auto scale = std::frexp(m, &e) * 256.f / m;
    out[0] = static_cast<uint8_t>(rgb[0] * scale);
    out[1] = static_cast<uint8_t>(rgb[1] * scale);
    out[2] = static_cast<uint8_t>(rgb[2] * scale);
    out[3] = static_cast<uint8_t>(e + 128);
}

// (nc = 1: the value as gray)
void write_hdr(const fs::path &path, const float *rgba, uint32_t w, uint32_t h, uint32_t nc = 4u) {
    std::ofstream f{path, std::ios::binary};
    if (!f) { throw Error{"Failed to save film to '" + path.string() + "'."}; }
    f << "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y " << h << " +X " << w << "\n";
    std::vector<uint8_t> line(static_cast<size_t>(w) * 4u);
    for (uint32_t y = 0; y < h; y++) {
        for (uint32_t x = 0; x < w; x++) {
            const auto px = rgba + (static_cast<size_t>(y) * w + x) * nc;
            const float gray[3] = {px[0], px[0], px[0]};
            float_to_rgbe(nc == 1u ? gray : px, &line[x * 4u]);
        }
        f.write(reinterpret_cast<const char *>(line.data()), static_cast<std::streamsize>(line.size()));
    }
}

float half_to_float(uint16_t hbits) {
    uint32_t sign = (hbits >> 15u) & 1u, exp = (hbits >> 10u) & 31u, man = hbits & 1023u;
    uint32_t f;
    if (exp == 0u) {
        if (man == 0u) { f = sign << 31u; }
        else {
            exp = 127u - 15u + 1u;
            while ((man & 1024u) == 0u) { man <<= 1u, exp--; }
            f = (sign << 31u) | (exp << 23u) | ((man & 1023u) << 13u);
        }
    } else if (exp == 31u) {
        f = (sign << 31u) | 0x7f800000u | (man << 13u);
    } else {
        f = (sign << 31u) | ((exp + 112u) << 23u) | (man << 13u);
    }
    float out;
    std::memcpy(&out, &f, 4);
    return out;
}

LoadedImage read_pfm(const fs::path &path) {
    std::ifstream f{path, std::ios::binary};
    if (!f) { throw Error{"Failed to load image '" + path.string() + "'."}; }
    std::string magic;
    int w, h;
    float scale;
    f >> magic >> w >> h >> scale;
    f.get();
    auto channels = magic == "PF" ? 3 : (magic == "Pf" ? 1 : (magic == "PF4" ? 4 : 0));
    if (channels == 0 || w <= 0 || h <= 0) { throw Error{"Invalid PFM image '" + path.string() + "'."}; }
    std::vector<float> raw(static_cast<size_t>(w) * static_cast<size_t>(h) * static_cast<size_t>(channels));
    f.read(reinterpret_cast<char *>(raw.data()), static_cast<std::streamsize>(raw.size() * 4u));
    if (scale > 0.f) {// big endian
        for (auto &v : raw) {
            uint32_t b;
            std::memcpy(&b, &v, 4);
            b = __builtin_bswap32(b);
            std::memcpy(&v, &b, 4);
        }
    }
    LoadedImage img;
    img.width = static_cast<uint32_t>(w), img.height = static_cast<uint32_t>(h);
    img.channels = static_cast<uint32_t>(channels), img.is_hdr = true;
    img.pixels.resize(static_cast<size_t>(w) * static_cast<size_t>(h) * 4u);
    for (auto y = 0; y < h; y++) {// PFM rows are bottom-to-top
        for (auto x = 0; x < w; x++) {
            auto src = &raw[(static_cast<size_t>(h - 1 - y) * static_cast<size_t>(w) + static_cast<size_t>(x)) * static_cast<size_t>(channels)];
            auto dst = &img.pixels[(static_cast<size_t>(y) * static_cast<size_t>(w) + static_cast<size_t>(x)) * 4u];
            dst[0] = src[0], dst[1] = channels >= 3 ? src[1] : 0.f, dst[2] = channels >= 3 ? src[2] : 0.f;
            dst[3] = channels == 4 ? src[3] : (channels == 1 ? 0.f : 1.f);
        }
    }
    return img;
}

LoadedImage read_hdr(const fs::path &path) {
    std::ifstream f{path, std::ios::binary};
    if (!f) { throw Error{"Failed to load image '" + path.string() + "'."}; }
    std::string line;
    std::getline(f, line);
    if (line.rfind("#?", 0) != 0) { throw Error{"Invalid Radiance HDR image '" + path.string() + "'."}; }
    while (std::getline(f, line) && !line.empty() && line != "\r") {}
    std::getline(f, line);
    int w = 0, h = 0;
    if (std::sscanf(line.c_str(), "-Y %d +X %d", &h, &w) != 2) { throw Error{"Unsupported HDR orientation in '" + path.string() + "'."}; }
    LoadedImage img;
    img.width = static_cast<uint32_t>(w), img.height = static_cast<uint32_t>(h), img.channels = 3u, img.is_hdr = true;
    img.pixels.resize(static_cast<size_t>(w) * static_cast<size_t>(h) * 4u);
    std::vector<uint8_t> scan(static_cast<size_t>(w) * 4u);
    for (auto y = 0; y < h; y++) {
        uint8_t head[4];
        f.read(reinterpret_cast<char *>(head), 4);
        if (head[0] == 2u && head[1] == 2u && (head[2] & 0x80u) == 0u && w >= 8 && w < 32768) {// new RLE
            for (auto c = 0; c < 4; c++) {
                auto x = 0;
                while (x < w) {
                    auto count = f.get();
                    if (count > 128) {
                        auto value = static_cast<uint8_t>(f.get());
                        count -= 128;
                        while (count-- > 0 && x < w) { scan[static_cast<size_t>(x++) * 4u + static_cast<size_t>(c)] = value; }
                    } else {
                        while (count-- > 0 && x < w) { scan[static_cast<size_t>(x++) * 4u + static_cast<size_t>(c)] = static_cast<uint8_t>(f.get()); }
                    }
                }
            }
        } else {// flat
            std::memcpy(scan.data(), head, 4);
            f.read(reinterpret_cast<char *>(scan.data() + 4), static_cast<std::streamsize>(scan.size() - 4u));
        }
        for (auto x = 0; x < w; x++) {
            auto p = &scan[static_cast<size_t>(x) * 4u];
            auto dst = &img.pixels[(static_cast<size_t>(y) * static_cast<size_t>(w) + static_cast<size_t>(x)) * 4u];
            if (p[3] == 0u) { dst[0] = dst[1] = dst[2] = 0.f; }
            else {
                auto s = std::ldexp(1.f, static_cast<int>(p[3]) - (128 + 8));
                dst[0] = static_cast<float>(p[0]) * s, dst[1] = static_cast<float>(p[1]) * s, dst[2] = static_cast<float>(p[2]) * s;
            }
            dst[3] = 1.f;
        }
    }
    return img;
}

// ---- OpenEXR PIZ (compression 4): per chunk of 32 scanlines, the 16-bit words of all channels (channel after channel) go
// through a value-compaction LUT, a 2-D Haar-like wavelet per channel plane and a canonical Huffman coder with a run-length
// symbol.  The reference reads it through tinyexr (src/util/imageio.cpp:419-538; tinyexr is an empty submodule in the snapshot);
// restated from the published OpenEXR format (ImfPizCompressor / ImfHuf / ImfWav) -- PARITY UNPINNED AGAINST REAL FILES: no PIZ
// file and no other decoder exist on this machine; tests/test_image_io.py holds it against an independent Python ENCODER of
// the same format description (round trips over the 14- and 16-bit wavelet paths, odd sizes, run-length symbols).
namespace piz {

struct Error {};// any inconsistency: the caller reports a corrupt chunk

struct BitReader {
    const uint8_t *p, *end;
    uint64_t c{0u};
    int lc{0};
    uint32_t get(int n) {// most significant bit first
        while (lc < n) {
            if (p >= end) { throw Error{}; }
            c = (c << 8u) | *p++;
            lc += 8;
        }
        lc -= n;
        return static_cast<uint32_t>((c >> lc) & ((1ull << n) - 1ull));
    }
};

constexpr uint32_t kEncSize = (1u << 16u) + 1u;// 65536 values + the run-length symbol
constexpr uint32_t kShortZeroRun = 59u, kLongZeroRun = 63u, kShortestLongRun = 2u + kLongZeroRun - kShortZeroRun;

// hufUncompress: header (min symbol, max symbol = run-length symbol, table bytes, data bits, reserved), 6-bit code lengths with
// zero runs, canonical codes (longest codes hold the numerically smallest values), data bits
void huffman_decode(const uint8_t *src, size_t size, uint16_t *out, size_t count) {
    if (size < 20u) { if (count != 0u) { throw Error{}; } return; }
    auto rd = [&](size_t at) { uint32_t v; std::memcpy(&v, src + at, 4); return v; };
    auto im = rd(0), iM = rd(4), n_bits = rd(12);
    if (im >= kEncSize || iM >= kEncSize || im > iM) { throw Error{}; }
    std::vector<uint8_t> length(kEncSize, 0u);
    BitReader table{src + 20u, src + size};
    for (auto i = im; i <= iM; i++) {
        auto l = table.get(6);
        if (l == kLongZeroRun || l >= kShortZeroRun) {
            auto run = l == kLongZeroRun ? table.get(8) + kShortestLongRun : l - kShortZeroRun + 2u;
            if (i + run > iM + 1u) { throw Error{}; }
            i += run - 1u;// (the lengths are zero already)
        } else {
            length[i] = static_cast<uint8_t>(l);
        }
    }
    const uint8_t *data = table.p;// the data starts at the next byte
    if (static_cast<uint64_t>(n_bits) > 8ull * static_cast<uint64_t>(src + size - data)) { throw Error{}; }
    // canonical codes: count per length, first code per length from the longest down, symbols in increasing order inside a length
    uint64_t count_of[59] = {}, first[59] = {};
    for (auto i = im; i <= iM; i++) { count_of[length[i]]++; }
    {
        uint64_t c = 0u;
        for (auto l = 58; l > 0; l--) {
            auto next = (c + count_of[l]) >> 1u;
            first[l] = c;
            c = next;
        }
    }
    std::vector<uint32_t> offset(60, 0u), symbols;
    for (auto l = 1; l <= 58; l++) { offset[l + 1] = offset[l] + static_cast<uint32_t>(count_of[l]); }
    symbols.resize(offset[59]);
    {
        auto fill = offset;
        for (auto i = im; i <= iM; i++) { if (length[i] != 0u) { symbols[fill[length[i]]++] = i; } }
    }
    // Short codes through a lookup table (round 3, ADVICE r02: the bit-serial walk below took up to 58 iterations per symbol and made
    // large PIZ environment maps slow to load): kLutBits bits of lookahead index a table of (symbol, length) for every code of at most
    // kLutBits bits -- in a PIZ stream nearly all symbols -- and only longer codes fall back to the walk, which starts at kLutBits + 1.
    constexpr int kLutBits = 12;
    struct Short {
        uint32_t symbol;
        uint8_t length;// 0: no code of <= kLutBits bits has this prefix
    };
    std::vector<Short> lut(size_t{1} << kLutBits, Short{0u, 0u});
    for (auto l = 1; l <= kLutBits; l++) {
        for (uint64_t k = 0; k < count_of[l]; k++) {
            const auto code = first[l] + k;
            if (code >> l) { throw Error{}; }// (an over-subscribed code table)
            const auto lo = code << (kLutBits - l);
            for (uint64_t fill = 0; fill < (uint64_t{1} << (kLutBits - l)); fill++) { lut[lo + fill] = Short{symbols[offset[l] + static_cast<uint32_t>(k)], static_cast<uint8_t>(l)}; }
        }
    }
    struct PeekReader {// the BitReader with a non-consuming look at the next bits (zero-padded behind the end of the stream)
        const uint8_t *p, *end;
        uint64_t c{0u};
        int lc{0};
        uint32_t peek(int n) {
            while (lc < n) {
                c = (c << 8u) | (p < end ? *p : 0u);
                p++;
                lc += 8;
            }
            return static_cast<uint32_t>((c >> (lc - n)) & ((1ull << n) - 1ull));
        }
        void skip(int n) { lc -= n; }
        uint32_t get(int n) { auto v = peek(n); skip(n); return v; }
    } bits{data, src + size};
    uint64_t used = 0u;
    size_t produced = 0u;
    const auto rlc = iM;
    auto emit = [&](uint32_t symbol) {
        if (symbol == rlc) {
            if (used + 8u > n_bits || produced == 0u) { throw Error{}; }
            auto run = bits.get(8);
            used += 8u;
            if (produced + run > count) { throw Error{}; }
            for (auto k = 0u; k < run; k++) { out[produced + k] = out[produced - 1u]; }
            produced += run;
        } else {
            if (produced >= count) { throw Error{}; }
            out[produced++] = static_cast<uint16_t>(symbol);
        }
    };
    while (used < n_bits) {
        const auto s = lut[bits.peek(kLutBits)];
        if (s.length != 0u && used + s.length <= n_bits) {
            bits.skip(s.length);
            used += s.length;
            emit(s.symbol);
            continue;
        }
        uint64_t code = 0u;
        auto found = false;
        for (auto l = 1; l <= 58 && used < n_bits; l++) {
            code = (code << 1u) | bits.get(1);
            used++;
            if (l > kLutBits && count_of[l] != 0u && code >= first[l] && code - first[l] < count_of[l]) {
                emit(symbols[offset[l] + static_cast<uint32_t>(code - first[l])]);
                found = true;
                break;
            }
        }
        if (!found) { throw Error{}; }
    }
    if (produced != count) { throw Error{}; }
}

inline void wdec14(uint16_t l, uint16_t h, uint16_t &a, uint16_t &b) {
    auto ls = static_cast<int16_t>(l), hs = static_cast<int16_t>(h);
    int hi = hs, ai = ls + (hi & 1) + (hi >> 1);
    a = static_cast<uint16_t>(static_cast<int16_t>(ai));
    b = static_cast<uint16_t>(static_cast<int16_t>(ai - hi));
}
inline void wdec16(uint16_t l, uint16_t h, uint16_t &a, uint16_t &b) {
    int m = l, d = h;
    auto bb = (m - (d >> 1)) & 0xffff;
    auto aa = (d + bb - 0x8000) & 0xffff;
    b = static_cast<uint16_t>(bb), a = static_cast<uint16_t>(aa);
}

// wav2Decode: the inverse 2-D wavelet of one plane (nx x ny words, strides ox / oy), coarsest level first
void wavelet_decode(uint16_t *in, int nx, int ox, int ny, int oy, uint16_t max_value) {
    const auto w14 = max_value < (1u << 14u);
    auto n = std::min(nx, ny);
    auto p = 1;
    while (p <= n) { p <<= 1; }
    p >>= 1;
    auto p2 = p;
    p >>= 1;
    auto dec = [&](uint16_t l, uint16_t h, uint16_t &a, uint16_t &b) { w14 ? wdec14(l, h, a, b) : wdec16(l, h, a, b); };
    while (p >= 1) {
        auto py = in;
        auto ey = in + static_cast<ptrdiff_t>(oy) * (ny - p2);
        auto oy1 = static_cast<ptrdiff_t>(oy) * p, oy2 = static_cast<ptrdiff_t>(oy) * p2;
        auto ox1 = static_cast<ptrdiff_t>(ox) * p, ox2 = static_cast<ptrdiff_t>(ox) * p2;
        uint16_t i00, i01, i10, i11;
        for (; py <= ey; py += oy2) {
            auto px = py;
            auto ex = py + static_cast<ptrdiff_t>(ox) * (nx - p2);
            for (; px <= ex; px += ox2) {
                auto p01 = px + ox1, p10 = px + oy1, p11 = p10 + ox1;
                dec(*px, *p10, i00, i10);
                dec(*p01, *p11, i01, i11);
                dec(i00, i01, *px, *p01);
                dec(i10, i11, *p10, *p11);
            }
            if (nx & p) {
                auto p10 = px + oy1;
                dec(*px, *p10, i00, *p10);
                *px = i00;
            }
        }
        if (ny & p) {
            auto px = py;
            auto ex = py + static_cast<ptrdiff_t>(ox) * (nx - p2);
            for (; px <= ex; px += ox2) {
                auto p01 = px + ox1;
                dec(*px, *p01, i00, *p01);
                *px = i00;
            }
        }
        p2 = p;
        p >>= 1;
    }
}

// one chunk -> the scanline layout of an uncompressed chunk (row after row, channel after channel inside a row).
// `words[c]`: 16-bit words per pixel of channel c (1 = HALF, 2 = FLOAT / UINT)
void decode_chunk(const uint8_t *src, size_t size, const std::vector<uint32_t> &words, uint32_t width, uint32_t rows, std::vector<uint8_t> &out) {
    size_t total = 0u;
    for (auto w : words) { total += static_cast<size_t>(w) * width * rows; }
    if (size < 4u) { throw Error{}; }
    uint16_t min_nz, max_nz;
    std::memcpy(&min_nz, src, 2), std::memcpy(&max_nz, src + 2, 2);
    constexpr size_t kBitmap = 8192u;
    if (max_nz >= kBitmap) { throw Error{}; }
    std::vector<uint8_t> bitmap(kBitmap, 0u);
    size_t at = 4u;
    if (min_nz <= max_nz) {
        auto n = static_cast<size_t>(max_nz - min_nz) + 1u;
        if (size - at < n) { throw Error{}; }
        std::memcpy(bitmap.data() + min_nz, src + at, n);
        at += n;
    }
    std::vector<uint16_t> lut(1u << 16u, 0u);
    uint32_t k = 0u;
    for (uint32_t i = 0u; i < (1u << 16u); i++) {// reverseLutFromBitmap: zero is always a value
        if (i == 0u || (bitmap[i >> 3u] & (1u << (i & 7u)))) { lut[k++] = static_cast<uint16_t>(i); }
    }
    const auto max_value = static_cast<uint16_t>(k - 1u);
    if (size - at < 4u) { throw Error{}; }
    int32_t length;
    std::memcpy(&length, src + at, 4);
    at += 4u;
    if (length < 0 || static_cast<size_t>(length) > size - at) { throw Error{}; }
    std::vector<uint16_t> buffer(total);
    huffman_decode(src + at, static_cast<size_t>(length), buffer.data(), total);
    size_t start = 0u;
    for (auto w : words) {
        for (auto j = 0u; j < w; j++) {
            wavelet_decode(buffer.data() + start + j, static_cast<int>(width), static_cast<int>(w), static_cast<int>(rows), static_cast<int>(width * w), max_value);
        }
        start += static_cast<size_t>(w) * width * rows;
    }
    for (auto &v : buffer) { v = lut[v]; }
    out.resize(total * 2u);
    std::vector<size_t> cursor(words.size());
    start = 0u;
    for (size_t c = 0; c < words.size(); c++) {
        cursor[c] = start;
        start += static_cast<size_t>(words[c]) * width * rows;
    }
    size_t q = 0u;
    for (uint32_t r = 0; r < rows; r++) {
        for (size_t c = 0; c < words.size(); c++) {
            auto n = static_cast<size_t>(words[c]) * width;
            std::memcpy(out.data() + q, buffer.data() + cursor[c], n * 2u);
            q += n * 2u, cursor[c] += n;
        }
    }
}

}// namespace piz

LoadedImage read_exr(const fs::path &path) {
    std::ifstream f{path, std::ios::binary};
    if (!f) { throw Error{"Failed to load image '" + path.string() + "'."}; }
    std::string data{std::istreambuf_iterator<char>{f}, std::istreambuf_iterator<char>{}};
    size_t p = 0;
    auto truncated = [&]() -> Error { return Error{"Truncated or corrupt EXR image '" + path.string() + "'."}; };
    auto need = [&](size_t at, size_t n) { if (at > data.size() || n > data.size() - at) { throw truncated(); } };
    auto rd32 = [&](size_t at) { need(at, 4u); uint32_t v; std::memcpy(&v, data.data() + at, 4); return v; };
    auto cstr = [&](size_t at) {// a NUL-terminated string that ends inside the file
        need(at, 1u);
        auto end = data.find('\0', at);
        if (end == std::string::npos) { throw truncated(); }
        return std::string{data.data() + at, end - at};
    };
    if (data.size() < 8u || rd32(0) != 20000630u) { throw Error{"Invalid EXR image '" + path.string() + "'."}; }
    if ((rd32(4) & 0x1e00u) != 0u) { throw Error{"Only single-part scanline EXR is supported: '" + path.string() + "'."}; }
    p = 8;
    struct Channel { std::string name; uint32_t type; };
    std::vector<Channel> channels;
    int32_t xmin = 0, ymin = 0, xmax = -1, ymax = -1;
    uint8_t compression = 0;
    while (p < data.size() && data[p] != '\0') {
        auto name = cstr(p);
        p += name.size() + 1u;
        auto type = cstr(p);
        p += type.size() + 1u;
        auto size = rd32(p);
        p += 4;
        need(p, size);
        if (name == "channels") {
            auto q = p;
            while (q < p + size && data[q] != '\0') {
                Channel c;
                c.name = cstr(q);
                q += c.name.size() + 1u;
                c.type = rd32(q);
                if (c.type > 2u) { throw truncated(); }
                q += 16u;
                channels.emplace_back(c);
            }
        } else if (name == "dataWindow") {
            need(p, 16u);
            std::memcpy(&xmin, data.data() + p, 4), std::memcpy(&ymin, data.data() + p + 4, 4);
            std::memcpy(&xmax, data.data() + p + 8, 4), std::memcpy(&ymax, data.data() + p + 12, 4);
        } else if (name == "compression") {
            need(p, 1u);
            compression = static_cast<uint8_t>(data[p]);
        }
        p += size;
    }
    p++;
    if (channels.empty() || xmax < xmin || ymax < ymin || static_cast<int64_t>(xmax) - xmin >= 65536 || static_cast<int64_t>(ymax) - ymin >= 65536) {
        throw Error{"Invalid EXR header (channels / dataWindow) in '" + path.string() + "'."};
    }
    // NO_COMPRESSION (0), ZIPS (2: one scanline per chunk), ZIP (3: 16 scanlines per chunk); the deflate streams go
    // through zlib (the reference reads EXR with tinyexr + miniz, src/util/imageio.cpp:419-538)
    // and RLE (1: one scanline per chunk; signed run bytes, then the same predictor + byte de-interleave as ZIP)
    // and PIZ (4: 32 scanlines per chunk; namespace piz above)
    // and PXR24 (5: 16 scanlines per chunk; a deflate stream of byte planes: per row and channel the most significant byte of every
    // pixel, then the next one ... -- 2 planes for HALF, 4 for UINT, 3 for FLOAT, whose low 8 mantissa bits the format drops -- each
    // value the difference to its left neighbour; restated from the published format, ImfPxr24Compressor; unpinned like PIZ)
    if (compression > 5u) {
        throw Error{"EXR compression " + std::to_string(compression) + " is not supported (NONE / RLE / ZIPS / ZIP / PIZ / PXR24 are): '" + path.string() + "'."};
    }
    auto w = static_cast<uint32_t>(xmax - xmin + 1), h = static_cast<uint32_t>(ymax - ymin + 1);
    // nothing is allocated on the word of the header alone: at most 2^28 pixels (the JPEG reader's cap), the file must be long
    // enough for the chunk-offset table and the 8-byte header of every chunk the data window promises, and the 16 bytes per decoded
    // pixel must be within what the file's bytes can expand to (8192 : 1 -- beyond deflate's 1032 : 1 and RLE's 64 : 1; a PIZ chunk
    // of one constant colour is the densest case): an 8 KB file claiming 16384 x 16384 no longer gets 4 GiB
    {
        const auto per_chunk = (compression == 3u || compression == 5u) ? 16u : (compression == 4u ? 32u : 1u);
        auto chunks = (static_cast<uint64_t>(h) + per_chunk - 1u) / per_chunk;
        if (static_cast<uint64_t>(w) * h > (1ull << 28u) || p > data.size() || (data.size() - p) / 16u < chunks ||
            static_cast<uint64_t>(w) * h * 16u > static_cast<uint64_t>(data.size()) * 8192u) {
            throw Error{"EXR data window " + std::to_string(w) + "x" + std::to_string(h) + " is too large for the file (or beyond 2^28 pixels): '" + path.string() + "'."};
        }
    }
    LoadedImage img;
    img.width = w, img.height = h, img.is_hdr = true;
    img.pixels.assign(static_cast<size_t>(w) * h * 4u, 0.f);
    auto has_alpha = false;
    uint32_t color_channels = 0u;
    size_t line_bytes = 0u;
    for (auto &c : channels) {
        if (c.name == "A") { has_alpha = true; } else { color_channels++; }
        line_bytes += static_cast<size_t>(w) * (c.type == 1u ? 2u : 4u);
    }
    img.channels = has_alpha ? 4u : std::min(color_channels, 3u);
    if (!has_alpha) {
        for (size_t i = 0; i < static_cast<size_t>(w) * h; i++) { img.pixels[i * 4u + 3u] = 1.f; }
    }
    auto lines_per_chunk = (compression == 3u || compression == 5u) ? 16u : (compression == 4u ? 32u : 1u);
    auto chunk_count = (h + lines_per_chunk - 1u) / lines_per_chunk;
    auto table = p;
    std::vector<uint8_t> raw, tmp;
    for (uint32_t chunk = 0; chunk < chunk_count; chunk++) {
        uint64_t off;
        need(table + static_cast<size_t>(chunk) * 8u, 8u);
        std::memcpy(&off, data.data() + table + static_cast<size_t>(chunk) * 8u, 8);
        if (off > data.size() || data.size() - off < 8u) { throw truncated(); }
        int32_t yy;
        uint32_t packed;
        std::memcpy(&yy, data.data() + off, 4);
        std::memcpy(&packed, data.data() + off + 4u, 4);
        if (yy < ymin || yy > ymax) { throw truncated(); }
        auto first_row = static_cast<uint32_t>(yy - ymin);
        auto rows = std::min(lines_per_chunk, h - first_row);
        auto expect = line_bytes * rows;
        auto src = reinterpret_cast<const uint8_t *>(data.data()) + off + 8u;
        if (packed > data.size() - off - 8u) { throw truncated(); }
        if (compression == 5u) {// PXR24: never stored raw (its planes are narrower than the pixels)
            size_t plane_bytes = 0u;
            for (auto &c : channels) { plane_bytes += static_cast<size_t>(w) * (c.type == 1u ? 2u : (c.type == 2u ? 3u : 4u)); }
            tmp.resize(plane_bytes * rows);
            uLongf out_len = static_cast<uLongf>(tmp.size());
            if (uncompress(tmp.data(), &out_len, src, packed) != Z_OK || out_len != tmp.size()) {
                throw Error{"Corrupt PXR24 chunk in EXR image '" + path.string() + "'."};
            }
            raw.resize(expect);
            size_t in = 0u, out = 0u;
            for (uint32_t r = 0; r < rows; r++) {
                for (auto &c : channels) {
                    const auto planes = c.type == 1u ? 2u : (c.type == 2u ? 3u : 4u);
                    uint32_t pixel = 0u;
                    for (uint32_t x = 0; x < w; x++) {
                        uint32_t diff = 0u;
                        for (auto k = 0u; k < planes; k++) { diff = (diff << 8u) | tmp[in + static_cast<size_t>(k) * w + x]; }
                        if (c.type == 2u) { diff <<= 8u; }// FLOAT: the three planes are the top 24 bits
                        pixel += diff;
                        if (c.type == 1u) {
                            auto hb = static_cast<uint16_t>(pixel);
                            std::memcpy(raw.data() + out, &hb, 2);
                            out += 2u;
                        } else {
                            std::memcpy(raw.data() + out, &pixel, 4);
                            out += 4u;
                        }
                    }
                    in += static_cast<size_t>(planes) * w;
                }
            }
        } else if (compression == 0u || packed == expect) {// stored
            if (packed < expect) { throw truncated(); }
            raw.assign(src, src + expect);
        } else {
            if (compression == 4u) {
                std::vector<uint32_t> words;
                for (auto &c : channels) { words.emplace_back(c.type == 1u ? 1u : 2u); }
                try {
                    piz::decode_chunk(src, packed, words, w, rows, raw);
                } catch (const piz::Error &) {
                    throw Error{"Corrupt PIZ chunk in EXR image '" + path.string() + "'."};
                }
                if (raw.size() != expect) { throw truncated(); }
            } else {
            tmp.resize(expect);
            if (compression == 1u) {// a count byte n: n >= 0 -> the next byte n + 1 times; n < 0 -> -n literal bytes
                size_t in = 0u, out = 0u;
                while (in < packed && out < expect) {
                    auto n = static_cast<int8_t>(src[in++]);
                    if (n < 0) {
                        auto count = static_cast<size_t>(-static_cast<int>(n));
                        if (in + count > packed || out + count > expect) { break; }
                        std::memcpy(tmp.data() + out, src + in, count);
                        in += count, out += count;
                    } else {
                        auto count = static_cast<size_t>(n) + 1u;
                        if (in >= packed || out + count > expect) { break; }
                        std::memset(tmp.data() + out, src[in++], count);
                        out += count;
                    }
                }
                if (out != expect) { throw Error{"Corrupt RLE chunk in EXR image '" + path.string() + "'."}; }
            } else {
            uLongf out_len = static_cast<uLongf>(expect);
            if (uncompress(tmp.data(), &out_len, src, packed) != Z_OK || out_len != expect) {
                throw Error{"Corrupt ZIP chunk in EXR image '" + path.string() + "'."};
            }
            }
            for (size_t i = 1; i < expect; i++) { tmp[i] = static_cast<uint8_t>(tmp[i - 1u] + tmp[i] - 128u); }// predictor
            raw.resize(expect);
            auto half = (expect + 1u) / 2u;// de-interleave: first half = even bytes, second half = odd bytes
            for (size_t i = 0; i < expect; i++) { raw[i] = (i & 1u) ? tmp[half + i / 2u] : tmp[i / 2u]; }
            }
        }
        size_t q = 0u;
        for (uint32_t r = 0; r < rows; r++) {
            auto row = first_row + r;
            for (auto &c : channels) {
                auto slot = c.name == "R" ? 0 : c.name == "G" ? 1 : c.name == "B" ? 2 : c.name == "A" ? 3 : (c.name == "Y" ? 0 : -1);
                auto bytes = c.type == 1u ? 2u : 4u;
                for (uint32_t x = 0; x < w; x++) {
                    float v;
                    if (c.type == 1u) {
                        uint16_t hb;
                        std::memcpy(&hb, raw.data() + q + static_cast<size_t>(x) * 2u, 2);
                        v = half_to_float(hb);
                    } else if (c.type == 2u) {
                        std::memcpy(&v, raw.data() + q + static_cast<size_t>(x) * 4u, 4);
                    } else {
                        uint32_t u;
                        std::memcpy(&u, raw.data() + q + static_cast<size_t>(x) * 4u, 4);
                        v = static_cast<float>(u);
                    }
                    if (slot >= 0) { img.pixels[(static_cast<size_t>(row) * w + x) * 4u + static_cast<size_t>(slot)] = v; }
                    if (c.name == "Y") {
                        img.pixels[(static_cast<size_t>(row) * w + x) * 4u + 1u] = v;
                        img.pixels[(static_cast<size_t>(row) * w + x) * 4u + 2u] = v;
                    }
                }
                q += static_cast<size_t>(w) * bytes;
            }
        }
    }
    return img;
}

// PNG (8 / 16 bit, grey / grey+alpha / RGB / RGBA / palette, non-interlaced): chunks -> zlib inflate -> scanline
// filters.  Values are returned in [0, 1] like stb_image's 8-bit path in the reference (imageio.cpp:500-538).
LoadedImage read_png(const fs::path &path) {
    std::ifstream f{path, std::ios::binary};
    if (!f) { throw Error{"Failed to load image '" + path.string() + "'."}; }
    std::string data{std::istreambuf_iterator<char>{f}, std::istreambuf_iterator<char>{}};
    static const unsigned char magic[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (data.size() < 8u || std::memcmp(data.data(), magic, 8) != 0) { throw Error{"Invalid PNG image '" + path.string() + "'."}; }
    auto be32 = [&](size_t at) {
        auto d = reinterpret_cast<const uint8_t *>(data.data()) + at;
        return (static_cast<uint32_t>(d[0]) << 24u) | (static_cast<uint32_t>(d[1]) << 16u) | (static_cast<uint32_t>(d[2]) << 8u) | d[3];
    };
    uint32_t w = 0, h = 0, depth = 0, color = 0, interlace = 0;
    std::vector<uint8_t> idat, palette, trns;
    for (size_t p = 8; p + 12u <= data.size();) {
        auto len = be32(p);
        std::string type{data.data() + p + 4u, 4u};
        auto body = reinterpret_cast<const uint8_t *>(data.data()) + p + 8u;
        if (len > data.size() || p + 12u + len > data.size()) { throw Error{"Truncated PNG image '" + path.string() + "'."}; }
        if (type == "IHDR") {
            if (len < 13u) { throw Error{"Corrupt PNG header '" + path.string() + "'."}; }
            w = be32(p + 8u), h = be32(p + 12u);
            depth = body[8], color = body[9], interlace = body[12];
        } else if (type == "PLTE") {
            palette.assign(body, body + len);
        } else if (type == "tRNS") {
            trns.assign(body, body + len);
        } else if (type == "IDAT") {
            idat.insert(idat.end(), body, body + len);
        } else if (type == "IEND") {
            break;
        }
        p += 12u + len;
    }
    if (w > 32768u || h > 32768u || (color != 0u && color != 2u && color != 3u && color != 4u && color != 6u) ||
        (color == 3u && depth != 1u && depth != 2u && depth != 4u && depth != 8u)) {
        throw Error{"Corrupt PNG header '" + path.string() + "'."};
    }
    if (w == 0u || h == 0u || interlace != 0u || (depth != 8u && depth != 16u && !(color == 3u && depth <= 8u))) {
        throw Error{"Unsupported PNG variant (interlaced or sub-byte samples) '" + path.string() + "'."};
    }
    auto samples = color == 0u ? 1u : color == 2u ? 3u : color == 3u ? 1u : color == 4u ? 2u : 4u;
    auto bpp = std::max(1u, samples * depth / 8u);// bytes per pixel for the filters
    auto stride = (static_cast<size_t>(w) * samples * depth + 7u) / 8u;
    std::vector<uint8_t> raw((stride + 1u) * h);
    uLongf out_len = static_cast<uLongf>(raw.size());
    if (uncompress(raw.data(), &out_len, idat.data(), static_cast<uLong>(idat.size())) != Z_OK || out_len != raw.size()) {
        throw Error{"Corrupt PNG data '" + path.string() + "'."};
    }
    std::vector<uint8_t> prev(stride, 0u), cur(stride);
    LoadedImage img;
    img.width = w, img.height = h, img.is_hdr = false;
    img.channels = color == 3u ? (trns.empty() ? 3u : 4u) : samples;
    img.pixels.assign(static_cast<size_t>(w) * h * 4u, 0.f);
    for (uint32_t y = 0; y < h; y++) {
        auto line = raw.data() + (stride + 1u) * y;
        auto filter = line[0];
        for (size_t i = 0; i < stride; i++) {
            int a = i >= bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0;
            int x = line[1u + i];
            switch (filter) {
                case 0: break;
                case 1: x += a; break;
                case 2: x += b; break;
                case 3: x += (a + b) / 2; break;
                case 4: {
                    auto pa = std::abs(b - c), pb = std::abs(a - c), pc = std::abs(a + b - 2 * c);
                    x += (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                    break;
                }
                default: throw Error{"Invalid PNG filter in '" + path.string() + "'."};
            }
            cur[i] = static_cast<uint8_t>(x);
        }
        auto sample = [&](uint32_t px, uint32_t s) {
            if (depth == 16u) {
                auto d = cur.data() + (static_cast<size_t>(px) * samples + s) * 2u;
                return static_cast<float>((d[0] << 8u) | d[1]) * (1.f / 65535.f);
            }
            return static_cast<float>(cur[static_cast<size_t>(px) * samples + s]) * (1.f / 255.f);
        };
        for (uint32_t x = 0; x < w; x++) {
            auto dst = img.pixels.data() + (static_cast<size_t>(y) * w + x) * 4u;
            dst[3] = 1.f;
            if (color == 3u) {
                uint32_t idx;
                if (depth == 8u) { idx = cur[x]; }
                else { idx = (cur[static_cast<size_t>(x) * depth / 8u] >> (8u - depth - (x * depth) % 8u)) & ((1u << depth) - 1u); }
                if (static_cast<size_t>(idx) * 3u + 2u < palette.size()) {
                    dst[0] = palette[idx * 3u] / 255.f, dst[1] = palette[idx * 3u + 1u] / 255.f, dst[2] = palette[idx * 3u + 2u] / 255.f;
                }
                if (idx < trns.size()) { dst[3] = trns[idx] / 255.f; }
            } else if (samples <= 2u) {
                dst[0] = dst[1] = dst[2] = sample(x, 0u);
                if (samples == 2u) { dst[3] = sample(x, 1u); }
            } else {
                dst[0] = sample(x, 0u), dst[1] = sample(x, 1u), dst[2] = sample(x, 2u);
                if (samples == 4u) { dst[3] = sample(x, 3u); }
            }
        }
        std::swap(prev, cur);
    }
    return img;
}

LoadedImage read_pnm(const fs::path &path) {
    std::ifstream f{path, std::ios::binary};
    if (!f) { throw Error{"Failed to load image '" + path.string() + "'."}; }
    std::string magic;
    f >> magic;
    auto next_int = [&] {
        for (;;) {
            f >> std::ws;
            if (f.peek() == '#') { std::string c; std::getline(f, c); } else { break; }
        }
        int v;
        f >> v;
        return v;
    };
    auto w = next_int(), h = next_int(), maxv = next_int();
    f.get();
    auto channels = magic == "P6" ? 3 : (magic == "P5" ? 1 : 0);
    if (channels == 0 || maxv != 255) { throw Error{"Unsupported PNM image '" + path.string() + "'."}; }
    std::vector<uint8_t> raw(static_cast<size_t>(w) * static_cast<size_t>(h) * static_cast<size_t>(channels));
    f.read(reinterpret_cast<char *>(raw.data()), static_cast<std::streamsize>(raw.size()));
    LoadedImage img;
    img.width = static_cast<uint32_t>(w), img.height = static_cast<uint32_t>(h), img.channels = static_cast<uint32_t>(channels);
    img.pixels.resize(static_cast<size_t>(w) * static_cast<size_t>(h) * 4u);
    for (size_t i = 0; i < static_cast<size_t>(w) * static_cast<size_t>(h); i++) {
        for (auto c = 0; c < 3; c++) {
            img.pixels[i * 4u + static_cast<size_t>(c)] = static_cast<float>(raw[i * static_cast<size_t>(channels) + static_cast<size_t>(channels == 3 ? c : 0)]) / 255.f;
        }
        img.pixels[i * 4u + 3u] = 1.f;
    }
    return img;
}

}// namespace

void save_image(const std::string &path_in, const float *rgba, uint32_t width, uint32_t height, uint32_t channels) {
    if (channels != 1u && channels != 3u && channels != 4u) { throw Error{"save_image: 1, 3 or 4 channels per pixel."}; }
    fs::path path{path_in};
    auto ext = lower_ext(path);
    if (ext != ".exr" && ext != ".hdr") {
        log_warning("Unsupported image extension '" + ext + "' in path '" + path.string() + "'. Falling back to '.exr'.");
        path.replace_extension(".exr");
        ext = ".exr";
    }
    if (auto folder = path.parent_path(); !folder.empty() && !fs::exists(folder)) { fs::create_directories(folder); }
    if (ext == ".exr") { write_exr(path, rgba, width, height, channels); } else { write_hdr(path, rgba, width, height, channels); }
}

LoadedImage load_image(const std::string &path_in) {
    fs::path path{path_in};
    auto ext = lower_ext(path);
    if (ext == ".pfm") { return read_pfm(path); }
    if (ext == ".hdr") { return read_hdr(path); }
    if (ext == ".exr") { return read_exr(path); }
    if (ext == ".ppm" || ext == ".pgm") { return read_pnm(path); }
    if (ext == ".png") { return read_png(path); }
    if (ext == ".jpg" || ext == ".jpeg") { return read_jpeg(path.string()); }
    if (ext == ".bmp") { return read_bmp(path.string()); }
    if (ext == ".tga") { return read_tga(path.string()); }
    throw Error{"Image format '" + ext + "' is not supported (stb is absent); supported: .pfm .hdr .exr (NONE/RLE/ZIPS/ZIP/PIZ/PXR24) .png .jpg .bmp .tga .ppm .pgm — '" +
                path.string() + "'."};
}

}// namespace lr
