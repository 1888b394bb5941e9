// pt_png.hpp -- a minimal PNG writer for pt_demo --png: 8-bit RGB (colour type 2; the frame's alpha is 0, so it is dropped), filter type
// 0 on every row, the image data in zlib stored (uncompressed) blocks, CRC-32 and Adler-32 computed here. Header-only, no dependencies.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace ptpng {

inline uint32_t crc32(const uint8_t* p, size_t n, uint32_t crc = 0)     // ISO 3309 / PNG: reflected 0xEDB88320
{
    static const std::vector<uint32_t> table = [] {
        std::vector<uint32_t> t(256);
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
        return t;
    }();
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xFFu] ^ (crc >> 8);
    return ~crc;
}

inline uint32_t adler32(const uint8_t* p, size_t n)                       // RFC 1950
{
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; i++) { a = (a + p[i]) % 65521u; b = (b + a) % 65521u; }
    return b << 16 | a;
}

inline void put32(std::vector<uint8_t>& v, uint32_t x) { for (int s = 24; s >= 0; s -= 8) v.push_back((uint8_t)(x >> s)); }

inline void chunk(std::vector<uint8_t>& out, const char type[4], const std::vector<uint8_t>& data)
{
    put32(out, (uint32_t)data.size());
    const size_t at = out.size();
    out.insert(out.end(), type, type + 4);
    out.insert(out.end(), data.begin(), data.end());
    put32(out, crc32(out.data() + at, data.size() + 4));
}

// rgba: width * height texels of 4 bytes, row-major, top row first (R8G8B8A8_UNORM as pt_post_render writes Display8)
inline std::vector<uint8_t> encode_rgb(const uint8_t* rgba, uint32_t width, uint32_t height)
{
    std::vector<uint8_t> raw;                                             // filter byte + RGB per row
    raw.reserve((size_t)height * (1 + 3 * (size_t)width));
    for (uint32_t y = 0; y < height; y++) {
        raw.push_back(0);
        for (uint32_t x = 0; x < width; x++) { const uint8_t* t = rgba + 4 * ((size_t)y * width + x); raw.insert(raw.end(), t, t + 3); }
    }
    std::vector<uint8_t> z = { 0x78, 0x01 };                              // deflate, 32 KiB window, no dictionary
    for (size_t at = 0; at < raw.size() || at == 0; ) {
        const size_t n = std::min<size_t>(65535, raw.size() - at);
        const bool last = at + n == raw.size();
        z.push_back(last ? 1 : 0);                                        // BFINAL, BTYPE 00 (stored)
        z.push_back((uint8_t)n); z.push_back((uint8_t)(n >> 8));
        z.push_back((uint8_t)~n); z.push_back((uint8_t)(~n >> 8));
        z.insert(z.end(), raw.begin() + at, raw.begin() + at + n);
        at += n;
        if (last) break;
    }
    put32(z, adler32(raw.data(), raw.size()));
    std::vector<uint8_t> out = { 0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n' };
    std::vector<uint8_t> ihdr;
    put32(ihdr, width); put32(ihdr, height);
    ihdr.insert(ihdr.end(), { 8, 2, 0, 0, 0 });                           // 8 bits, truecolour, deflate, filter method 0, no interlace
    chunk(out, "IHDR", ihdr);
    chunk(out, "IDAT", z);
    chunk(out, "IEND", {});
    return out;
}

inline bool write_rgb(const std::string& path, const uint8_t* rgba, uint32_t width, uint32_t height)
{
    const std::vector<uint8_t> png = encode_rgb(rgba, width, height);
    FILE* fp = fopen(path.c_str(), "wb");
    if (!fp) return false;
    const bool ok = fwrite(png.data(), 1, png.size(), fp) == png.size();
    return fclose(fp) == 0 && ok;
}

} // namespace ptpng
