// pt_ingest.hpp -- scene-JSON + glTF 2.0 ingest for the C++ host, in the reference's schema and conventions.
//
// What it mirrors (host side of the path, upstream of the acceleration-structure build):
//   scene descriptor   Source/MyScene.ixx:33-90, Source/JSONConverters.ixx:12-33, Source/Scene.ixx:33-73
//                      {Camera{Position,Rotation}, EnvironmentLight{Color,Rotation,Texture}, Models{name:path},
//                       RenderObjects[{Name,Transform{Translation,Rotation,Scale},IsVisible,Model,Animation}], Animations{name:path}}
//   animations         Source/GLTFHelpers.ixx:278-345, 463-520 (JOINTS_0 / WEIGHTS_0, skins) and :539-663 (LoadAnimation): load_animation below
//   glTF loader        Source/GLTFHelpers.ixx:142-537 (ProcessPrimitive, LoadModel): triangles only, the index array written BACKWARDS
//                      (flipWindingOrder is always set, Scene.ixx:90), u16 indices iff count <= 65535, tangents ALWAYS recomputed when
//                      NORMAL + TEXCOORD_0 exist, material factors incl. KHR_materials_emissive_strength / ior / transmission
//   instance transform Source/Scene.ixx:195-231: world = GlobalTransform * Scale(1,1,-1) * RenderObject.Transform() (row vectors),
//                      AffineTransform = Scale * Rotation * Translation (Math.ixx:17-19)
// Same conventions, same arithmetic order as the test harness's ingest.py, so that both hosts hand the library the same bytes
// (tests/test_host_cpp.py compares vertex / index buffers, transforms and materials of the committed fixture, and the rendered frame).
// Textures: 8-bit PNG images (embedded or referenced) are decoded here (a small inflate + the PNG filters, checked against PIL); the reference
// decodes files with DirectXTex / stb behind TextureHelpers.ixx, this image has neither, so JPEG / 16-bit references are listed in
// MeshData::SkippedTextures and the material keeps its factors (a host with a codec fills those slots through pt_heap_set_texture).
// DDS images -- a texture's MSFT_texture_dds source wins over its PNG, as in the reference -- need no codec: the header is parsed here
// and the BC1 / BC3 / BC4 / BC5 blocks go to the library as they are (read_dds below); a DDS outside those formats is listed and skipped too.
// [DirectXMesh spec] ComputeTangentFrame is an un-vendored dependency: restated as Lengyel's per-vertex accumulation with Gram-Schmidt
// against the normal (as in ingest.py). Header-only, C++20, no dependency beyond the standard library and include/ptamd.h.
//
// These are the only files the project reads that it did not write, so every size, offset and index a file states passes one of the checked
// primitives at the top before it is used: Bytes (a view that refuses a read outside itself), Json::uint / index / string / real (a value of
// the right kind and range, or a refusal) and add / mul (size arithmetic that refuses to wrap). Below them nothing touches a raw file byte or
// turns a JSON number into an integer, with one exception: Asset::element reads inside a range that Asset::accessor has validated, once per
// vertex component. What the hosts accept is stated in DESIGN.md section 2; every refusal is a std::runtime_error.
#pragma once
#include <array>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ptamd.h"

namespace ptamd::ingest {

// ------------------------------------------------------------------------------------------------
// checked primitives: size arithmetic, a byte view, JSON values
// ------------------------------------------------------------------------------------------------
inline size_t add(size_t a, size_t b) { if (b > SIZE_MAX - a) throw std::runtime_error("a size stated by the file overflows"); return a + b; }
inline size_t mul(size_t a, size_t b) { if (b && a > SIZE_MAX / b) throw std::runtime_error("a size stated by the file overflows"); return a * b; }

// a non-owning view of file bytes; every read names an offset and a length and throws unless both lie inside the view
struct Bytes {
    const uint8_t* data = nullptr; size_t size = 0;
    Bytes() = default;
    Bytes(const uint8_t* p, size_t n) : data(p), size(n) {}
    Bytes(const std::string& s) : data(reinterpret_cast<const uint8_t*>(s.data())), size(s.size()) {}
    Bytes(const std::vector<uint8_t>& v) : data(v.data()), size(v.size()) {}

    Bytes sub(size_t off, size_t len, const char* what = "a read") const
    {
        if (len > size || off > size - len)                                // never off + len: it may wrap
            throw std::runtime_error(std::string(what) + " of " + std::to_string(len) + " bytes at offset " + std::to_string(off) + " reaches beyond the " + std::to_string(size) + " bytes there are");
        return Bytes(data + off, len);
    }
    Bytes from(size_t off) const { return sub(off, off <= size ? size - off : 0); }
    uint8_t u8(size_t off) const { return sub(off, 1).data[0]; }
    uint16_t le16(size_t off) const { const uint8_t* p = sub(off, 2).data; return (uint16_t)(p[0] | (p[1] << 8)); }
    uint32_t le32(size_t off) const { const uint8_t* p = sub(off, 4).data; return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
    uint32_t be32(size_t off) const { const uint8_t* p = sub(off, 4).data; return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
    bool is(const char* s) const { return size == std::strlen(s) && !std::memcmp(data, s, size); }
    bool starts_with(const char* s, size_t n) const { return size >= n && !std::memcmp(data, s, n); }
    const uint8_t* begin() const { return data; }
    const uint8_t* end() const { return data + size; }
    void append_to(std::vector<uint8_t>& v) const { v.insert(v.end(), begin(), end()); }
};

// objects, arrays, strings, numbers, true / false / null. The public members are what JsonParser fills; file content is read through the
// accessors, which throw on a value of the wrong kind (a bare .num / .str would silently give 0 / "").
struct Json {
    enum Kind { Null, Bool, Number, String, Array, Object } kind = Null;
    bool b = false; double num = 0.0; std::string str;
    std::vector<Json> arr; std::vector<std::pair<std::string, Json>> obj;

    const Json* find(const std::string& key) const
    {
        if (kind != Object) return nullptr;
        for (auto& kv : obj) if (kv.first == key) return &kv.second;
        return nullptr;
    }
    bool has(const std::string& key) const { const Json* j = find(key); return j && j->kind != Null; }
    const Json& at(const std::string& key) const { const Json* j = find(key); if (!j) throw std::runtime_error("JSON: missing key " + key); return *j; }
    const Json& at(size_t i) const { if (kind != Array || i >= arr.size()) throw std::runtime_error("JSON: index out of range"); return arr[i]; }
    const std::vector<Json>& items() const { if (kind != Array) throw std::runtime_error("JSON: an array is expected"); return arr; }
    size_t size() const { return kind == Array ? arr.size() : obj.size(); }

    double real() const { if (kind != Number) throw std::runtime_error("JSON: a number is expected"); return num; }
    double number(const std::string& key, double def) const { const Json* j = find(key); return j && j->kind == Number ? j->num : def; }
    float f32() const { return (float)real(); }
    float f32(const std::string& key, double def) const { return (float)number(key, def); }
    const std::string& string() const { if (kind != String) throw std::runtime_error("JSON: a string is expected"); return str; }
    // the one place a JSON number becomes an integer: finite, integral, 0 <= value <= max (and <= 2^53: up to there a double holds every integer)
    size_t uint(size_t max) const
    {
        if (kind != Number || !(num >= 0.0) || !(num <= (double)(max < kMaxUint ? max : kMaxUint)) || num != std::floor(num))
            throw std::runtime_error("JSON: " + (kind == Number ? std::to_string(num) : std::string("a value that is no number")) + " where an integer from 0 to " + std::to_string(max) + " is expected");
        return (size_t)num;
    }
    size_t uint(const std::string& key, size_t def, size_t max) const { const Json* j = find(key); return j ? j->uint(max) : def; }   // an optional member
    size_t index(size_t limit) const { if (!limit) throw std::runtime_error("JSON: an index into an empty list"); return uint(limit - 1); }
    const Json& pick(const Json& i) const { return items()[i.index(arr.size())]; }   // the element of this list that the file value i names
    static constexpr size_t kMaxUint = (size_t)1 << 53;
};

// Nesting limit of the reader, which recurses once per level. Measured: the deepest nesting in tests/golden/ingest/* and in what
// ingest.export_scene writes is 6 (document -> materials -> material -> extensions -> extension -> texture info); the reader without a limit,
// built with -O1 under AddressSanitizer, overflows the default 8 MiB stack at a nesting of 9688. A power of two that is at least 4 x 6 and
// at most 9688 / 4; ingest.py has the same limit (MAX_JSON_DEPTH).
constexpr int kMaxJsonDepth = 128;

class JsonParser {
public:
    explicit JsonParser(Bytes text) : s(text) {}
    Json parse() { Json v = value(1); ws(); if (p != s.size) fail("trailing characters"); return v; }

private:
    const Bytes s; size_t p = 0; std::string token;
    [[noreturn]] void fail(const std::string& what) const { throw std::runtime_error("JSON: " + what + " at byte " + std::to_string(p)); }
    int peek() const { return p < s.size ? s.u8(p) : -1; }                 // -1: the end of the text
    void ws() { for (int c = peek(); c == ' ' || c == '\n' || c == '\t' || c == '\r'; c = peek()) p++; }
    bool eat(char c) { ws(); if (peek() == c) { p++; return true; } return false; }
    bool word(const char* w, size_t n) { if (n > s.size - p || !s.sub(p, n).is(w)) return false; p += n; return true; }
    unsigned hex4()
    {
        unsigned cp = 0;
        for (int k = 0; k < 4; k++, p++) {
            const int c = peek(), d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
            if (d < 0) fail("bad \\u escape");
            cp = cp * 16 + (unsigned)d;
        }
        return cp;
    }
    Json value(int depth)
    {
        ws();
        Json v;
        const int c = peek();
        if (c < 0) fail("unexpected end");
        if ((c == '{' || c == '[') && depth > kMaxJsonDepth) fail("arrays and objects nested deeper than " + std::to_string(kMaxJsonDepth));
        if (c == '{') {
            p++; v.kind = Json::Object;
            if (eat('}')) return v;
            do { ws(); Json k = value(depth + 1); if (k.kind != Json::String) fail("object key is not a string"); if (!eat(':')) fail("':' expected"); v.obj.emplace_back(std::move(k.str), value(depth + 1)); } while (eat(','));
            if (!eat('}')) fail("'}' expected");
        } else if (c == '[') {
            p++; v.kind = Json::Array;
            if (eat(']')) return v;
            do v.arr.push_back(value(depth + 1)); while (eat(','));
            if (!eat(']')) fail("']' expected");
        } else if (c == '"') {
            p++; v.kind = Json::String;
            for (int ch = peek(); ch != '"'; ch = peek()) {
                if (ch < 0) fail("unterminated string");
                p++;
                if (ch != '\\') { v.str += (char)ch; continue; }
                const int e = peek();
                if (e < 0) fail("bad escape");
                p++;
                switch (e) {
                case 'n': v.str += '\n'; break; case 't': v.str += '\t'; break; case 'r': v.str += '\r'; break;
                case 'b': v.str += '\b'; break; case 'f': v.str += '\f'; break;
                case 'u': {                                                // BMP code point -> UTF-8 (names and paths only)
                    const unsigned cp = hex4();
                    if (cp < 0x80) v.str += (char)cp;
                    else if (cp < 0x800) { v.str += (char)(0xC0 | (cp >> 6)); v.str += (char)(0x80 | (cp & 0x3F)); }
                    else { v.str += (char)(0xE0 | (cp >> 12)); v.str += (char)(0x80 | ((cp >> 6) & 0x3F)); v.str += (char)(0x80 | (cp & 0x3F)); }
                    break; }
                default: v.str += (char)e;
                }
            }
            p++;
        } else if (word("true", 4)) { v.kind = Json::Bool; v.b = true; }
        else if (word("false", 5)) { v.kind = Json::Bool; v.b = false; }
        else if (word("null", 4)) { v.kind = Json::Null; }
        else {                                                             // a number: the JSON token, then strtod on a copy of it alone (so no "nan", "inf" or hex,
            token.clear();                                                 // and nothing read past the end of a view that no NUL ends)
            for (int ch = c; (ch >= '0' && ch <= '9') || ch == '-' || ch == '+' || ch == '.' || ch == 'e' || ch == 'E'; ch = peek()) { token += (char)ch; p++; }
            if (c != '-' && !(c >= '0' && c <= '9')) fail("value expected");
            char* end = nullptr;
            v.num = std::strtod(token.c_str(), &end);                      // correctly rounded, like Python's float()
            if (token.empty() || end != token.c_str() + token.size()) fail("bad number");
            v.kind = Json::Number;
        }
        return v;
    }
};

inline std::string read_file(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
inline std::string dir_of(const std::string& path) { const size_t k = path.find_last_of('/'); return k == std::string::npos ? std::string(".") : path.substr(0, k); }
inline std::string resolve(const std::string& base, const std::string& p) { return (p.empty() || p[0] == '/') ? p : base + "/" + p; }

inline std::string base64_decode(Bytes in)
{
    std::string out; unsigned acc = 0; int bits = 0;
    for (unsigned char c : in) {
        int v;
        if (c >= 'A' && c <= 'Z') v = c - 'A'; else if (c >= 'a' && c <= 'z') v = c - 'a' + 26; else if (c >= '0' && c <= '9') v = c - '0' + 52;
        else if (c == '+' || c == '-') v = 62; else if (c == '/' || c == '_') v = 63; else continue;     // '=' padding and whitespace are skipped
        acc = (acc << 6) | (unsigned)v; bits += 6;
        if (bits >= 8) { bits -= 8; out += (char)((acc >> bits) & 0xFFu); }
    }
    return out;
}
// what a buffer's or an image's uri names: the payload of a data: uri, or the file beside the model
inline std::string read_uri(const std::string& dir, const std::string& uri)
{
    if (uri.compare(0, 5, "data:")) return read_file(resolve(dir, uri));
    const size_t comma = uri.find(',');
    return base64_decode(Bytes(uri).from(comma == std::string::npos ? 0 : comma + 1));
}

// ------------------------------------------------------------------------------------------------
// PNG (the lossless half of what glTF embeds; JPEG needs a codec this image does not have: such textures are listed and skipped)
// ------------------------------------------------------------------------------------------------
// RFC 1951 inflate (stored, fixed and dynamic Huffman blocks) behind the RFC 1950 zlib header; canonical-code decoding by counts per length.
class Inflate {
public:
    // expected: the size the caller knows the stream must inflate to; one that produces more is refused as soon as it does, so the output
    // is bounded by what the image header and the file's own bytes justify
    static std::vector<uint8_t> zlib(Bytes src, size_t expected)
    {
        if (src.size < 6 || (src.u8(0) & 0x0F) != 8 || ((src.u8(0) << 8) | src.u8(1)) % 31 != 0 || (src.u8(1) & 0x20)) throw std::runtime_error("PNG: bad zlib header");
        Inflate z(src.from(2), expected);
        z.run();
        return std::move(z.out);
    }

private:
    Inflate(Bytes s, size_t expected) : in(s), limit(expected) {}
    const Bytes in; const size_t limit; size_t pos = 0; uint32_t bitbuf = 0; int bitcnt = 0;
    std::vector<uint8_t> out;
    void room(size_t n) const { if (n > limit - out.size()) throw std::runtime_error("PNG: the deflate stream holds more than the image needs"); }
    struct Huffman { uint16_t count[16]; uint16_t symbol[288]; };

    uint32_t bits(int need)
    {
        uint32_t v = bitbuf;
        while (bitcnt < need) { v |= (uint32_t)in.u8(pos++) << bitcnt; bitcnt += 8; }         // (the view refuses a read past the end of the stream)
        bitbuf = need < 32 ? v >> need : 0; bitcnt -= need;
        return need < 32 ? v & ((1u << need) - 1u) : v;
    }
    static void build(Huffman& h, const uint8_t* lengths, int n)
    {
        for (int i = 0; i < 16; i++) h.count[i] = 0;
        for (int i = 0; i < n; i++) h.count[lengths[i]]++;
        uint16_t offs[16]; offs[1] = 0;
        for (int i = 1; i < 15; i++) offs[i + 1] = (uint16_t)(offs[i] + h.count[i]);
        for (int i = 0; i < n; i++) if (lengths[i]) h.symbol[offs[lengths[i]]++] = (uint16_t)i;
        h.count[0] = 0;
    }
    int decode(const Huffman& h)
    {
        int code = 0, first = 0, index = 0;
        for (int len = 1; len <= 15; len++) {
            code |= (int)bits(1);
            const int count = h.count[len];
            if (code - count < first) return h.symbol[index + (code - first)];
            index += count; first += count; first <<= 1; code <<= 1;
        }
        throw std::runtime_error("PNG: bad Huffman code");
    }
    void codes(const Huffman& lencode, const Huffman& distcode)
    {
        static const uint16_t lbase[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
        static const uint16_t lext[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0 };
        static const uint16_t dbase[30] = { 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577 };
        static const uint16_t dext[30] = { 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13 };
        for (;;) {
            int sym = decode(lencode);
            if (sym < 256) { room(1); out.push_back((uint8_t)sym); }
            else if (sym == 256) return;
            else {
                sym -= 257;
                if (sym >= 29) throw std::runtime_error("PNG: bad length symbol");
                const int len = lbase[sym] + (int)bits(lext[sym]);
                const int ds = decode(distcode);
                if (ds >= 30) throw std::runtime_error("PNG: bad distance symbol");
                const size_t dist = dbase[ds] + bits(dext[ds]);
                if (dist > out.size()) throw std::runtime_error("PNG: distance beyond the window");
                room((size_t)len);
                for (int k = 0; k < len; k++) out.push_back(out[out.size() - dist]);
            }
        }
    }
    void run()
    {
        for (bool last = false; !last;) {
            last = bits(1) != 0;
            const uint32_t type = bits(2);
            if (type == 0) {
                bitbuf = 0; bitcnt = 0;
                const uint32_t len = in.le16(pos), nlen = in.le16(pos + 2);  // pos <= in.size: no wrap
                pos += 4;
                if ((len ^ 0xFFFFu) != nlen) throw std::runtime_error("PNG: bad stored block");
                room(len);
                in.sub(pos, len, "PNG: a stored block").append_to(out); pos += len;
            } else if (type == 1) {
                uint8_t l[288];
                for (int i = 0; i < 288; i++) l[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
                Huffman lc, dc; build(lc, l, 288);
                uint8_t d[30]; for (int i = 0; i < 30; i++) d[i] = 5;
                build(dc, d, 30);
                codes(lc, dc);
            } else if (type == 2) {
                static const uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
                const int nlen = (int)bits(5) + 257, ndist = (int)bits(5) + 1, ncode = (int)bits(4) + 4;
                if (nlen > 286 || ndist > 30) throw std::runtime_error("PNG: bad dynamic block header");
                uint8_t l[320] = { 0 };
                for (int i = 0; i < ncode; i++) l[order[i]] = (uint8_t)bits(3);
                Huffman cl; build(cl, l, 19);
                uint8_t lengths[320]; int idx = 0;
                while (idx < nlen + ndist) {
                    int sym = decode(cl);
                    if (sym < 16) lengths[idx++] = (uint8_t)sym;
                    else {
                        uint8_t prev = 0; int rep;
                        if (sym == 16) { if (!idx) throw std::runtime_error("PNG: repeat without a previous length"); prev = lengths[idx - 1]; rep = 3 + (int)bits(2); }
                        else if (sym == 17) rep = 3 + (int)bits(3); else rep = 11 + (int)bits(7);
                        if (idx + rep > nlen + ndist) throw std::runtime_error("PNG: too many code lengths");
                        while (rep--) lengths[idx++] = prev;
                    }
                }
                Huffman lc, dc; build(lc, lengths, nlen); build(dc, lengths + nlen, ndist);
                codes(lc, dc);
            } else throw std::runtime_error("PNG: bad block type");
        }
    }
};

struct Image { uint32_t Width = 0, Height = 0; std::vector<uint8_t> RGBA; };       // 8 bits per channel, rows top to bottom

inline bool is_png(Bytes d) { return d.starts_with("\x89PNG\r\n\x1a\n", 8); }
constexpr uint32_t kMaxImageSide = 65536;                                  // of a PNG and of a DDS alike (D3D12's limit is 16384)

// 8-bit grey / grey+alpha / RGB / RGBA / palette PNG without interlacing -> RGBA8, as PIL's Image.open(...).convert("RGBA") delivers it
inline Image decode_png(Bytes d)
{
    if (!is_png(d)) throw std::runtime_error("not a PNG");
    Image im; int depth = 0, ctype = 0, interlace = 0;
    std::vector<uint8_t> idat; Bytes palette, trns;
    for (size_t o = 8; d.size - o >= 12;) {                                 // length, type, body, CRC
        const Bytes chunk = d.sub(o, add(12, d.be32(o)), "PNG: a chunk"), type = chunk.sub(4, 4), body = chunk.sub(8, chunk.size - 12);
        if (type.is("IHDR")) {
            if (body.size != 13) throw std::runtime_error("PNG: IHDR is not 13 bytes");
            im.Width = body.be32(0); im.Height = body.be32(4); depth = body.u8(8); ctype = body.u8(9); interlace = body.u8(12);
        }
        else if (type.is("PLTE")) palette = body;
        else if (type.is("tRNS")) trns = body;
        else if (type.is("IDAT")) body.append_to(idat);
        else if (type.is("IEND")) break;
        o += chunk.size;
    }
    const int channels = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    if (!channels || depth != 8 || interlace || !im.Width || !im.Height) throw std::runtime_error("PNG: only 8-bit non-interlaced images are decoded here");
    if (im.Width > kMaxImageSide || im.Height > kMaxImageSide) throw std::runtime_error("PNG: image larger than 65536 texels a side");
    const size_t bpp = (size_t)channels, stride = mul(im.Width, bpp), texels = mul(im.Width, im.Height);
    const std::vector<uint8_t> raw = Inflate::zlib(idat, mul(add(stride, 1), im.Height));     // no more than this; every buffer below is sized
    if (raw.size() < mul(add(stride, 1), im.Height)) throw std::runtime_error("PNG: image data too short");   // once that much data exists
    std::vector<uint8_t> px(mul(stride, im.Height));
    for (uint32_t y = 0; y < im.Height; y++) {                                      // undo the scanline filters (PNG spec 9.2)
        const uint8_t* src = raw.data() + (stride + 1) * y; const int f = src[0]; src++;
        uint8_t* cur = px.data() + stride * y; const uint8_t* up = y ? cur - stride : nullptr;
        for (size_t x = 0; x < stride; x++) {
            const int a = x >= bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
            int v = src[x];
            if (f == 1) v += a; else if (f == 2) v += b; else if (f == 3) v += (a + b) >> 1;
            else if (f == 4) { const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c); v += (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); }
            else if (f != 0) throw std::runtime_error("PNG: bad filter type");
            cur[x] = (uint8_t)v;
        }
    }
    im.RGBA.resize(mul(texels, 4));
    for (size_t i = 0; i < texels; i++) {
        uint8_t* o = im.RGBA.data() + 4 * i; const uint8_t* s = px.data() + bpp * i;
        if (ctype == 6) { o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3]; }
        else if (ctype == 2) { o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = 255; }
        else if (ctype == 0) { o[0] = o[1] = o[2] = s[0]; o[3] = 255; }
        else if (ctype == 4) { o[0] = o[1] = o[2] = s[0]; o[3] = s[1]; }
        else { const size_t k = s[0]; const Bytes rgb = palette.sub(3 * k, 3, "PNG: a palette entry");
               o[0] = rgb.u8(0); o[1] = rgb.u8(1); o[2] = rgb.u8(2); o[3] = k < trns.size ? trns.u8(k) : 255; }
    }
    return im;
}

// ------------------------------------------------------------------------------------------------
// DDS (mip 0 of a 2D texture): header parsing only, the blocks are passed through as they are (the reference hands them to the GPU the
// same way, TextureHelpers.ixx:65-78). The same acceptance as the harness's bc.read_dds: the DX10 header with DXGI 28, 29, 71, 72, 77, 78,
// 80, 83, the FourCCs DXT1, DXT5, ATI1 / BC4U, ATI2 / BC5U, and 32-bit RGBA masks; everything else throws. Every size the file states is
// checked against the buffer before a byte is read.
// ------------------------------------------------------------------------------------------------
inline bool is_dds(Bytes d) { return d.starts_with("DDS ", 4); }

struct DdsImage { uint32_t Width = 0, Height = 0, Format = 0; std::vector<uint8_t> Data; };   // Format: PtFormat; Data: blocks, or RGBA8 texels

inline DdsImage read_dds(Bytes d)
{
    if (!is_dds(d)) throw std::runtime_error("DDS: no 'DDS ' magic");
    if (d.size < 128) throw std::runtime_error("DDS: the file is shorter than its header");
    const uint32_t size = d.le32(4), flags = d.le32(8), height = d.le32(12), width = d.le32(16), depth = d.le32(24), pfSize = d.le32(76), pfFlags = d.le32(80), caps2 = d.le32(112);
    uint32_t mips = d.le32(28);
    if (size != 124 || pfSize != 32) throw std::runtime_error("DDS: bad header size");
    if (!width || !height) throw std::runtime_error("DDS: zero width or height");
    if (width > kMaxImageSide || height > kMaxImageSide) throw std::runtime_error("DDS: texture larger than 65536 texels a side");
    if ((caps2 & 0x200000u) || ((flags & 0x800000u) && depth > 1)) throw std::runtime_error("DDS: volume textures are not supported");
    if (caps2 & 0x200u) throw std::runtime_error("DDS: cube maps are not supported");
    DdsImage im; im.Width = width; im.Height = height;
    size_t off = 128;
    const bool fourcc = (pfFlags & 0x4u) != 0;
    const Bytes cc = d.sub(84, 4);
    if (fourcc && cc.is("DX10")) {
        if (d.size < 148) throw std::runtime_error("DDS: the file is shorter than its DX10 header");
        const uint32_t dxgi = d.le32(128), dimension = d.le32(132), misc = d.le32(136), arraySize = d.le32(140);
        off = 148;
        if (dimension == 4) throw std::runtime_error("DDS: volume textures are not supported");
        if (dimension != 3) throw std::runtime_error("DDS: only 2D textures are supported");
        if (misc & 0x4u) throw std::runtime_error("DDS: cube maps are not supported");
        if (arraySize > 1) throw std::runtime_error("DDS: texture arrays are not supported");
        switch (dxgi) {
        case 28: im.Format = PT_FORMAT_R8G8B8A8_UNORM; break; case 29: im.Format = PT_FORMAT_R8G8B8A8_UNORM_SRGB; break;
        case 71: im.Format = PT_FORMAT_BC1_UNORM; break; case 72: im.Format = PT_FORMAT_BC1_UNORM_SRGB; break;
        case 77: im.Format = PT_FORMAT_BC3_UNORM; break; case 78: im.Format = PT_FORMAT_BC3_UNORM_SRGB; break;
        case 80: im.Format = PT_FORMAT_BC4_UNORM; break; case 83: im.Format = PT_FORMAT_BC5_UNORM; break;
        default: throw std::runtime_error("DDS: unsupported DXGI format " + std::to_string(dxgi));
        }
    } else if (fourcc) {
        if (cc.is("DXT1")) im.Format = PT_FORMAT_BC1_UNORM; else if (cc.is("DXT5")) im.Format = PT_FORMAT_BC3_UNORM;
        else if (cc.is("ATI1") || cc.is("BC4U")) im.Format = PT_FORMAT_BC4_UNORM; else if (cc.is("ATI2") || cc.is("BC5U")) im.Format = PT_FORMAT_BC5_UNORM;
        else throw std::runtime_error("DDS: unsupported FourCC");
    } else if ((pfFlags & 0x40u) && (pfFlags & 0x1u) && d.le32(88) == 32 && d.le32(92) == 0xFFu && d.le32(96) == 0xFF00u && d.le32(100) == 0xFF0000u && d.le32(104) == 0xFF000000u)
        im.Format = PT_FORMAT_R8G8B8A8_UNORM;
    else throw std::runtime_error("DDS: unsupported pixel format");
    const bool block = im.Format >= PT_FORMAT_BC1_UNORM;
    const size_t blockBytes = (im.Format == PT_FORMAT_BC3_UNORM || im.Format == PT_FORMAT_BC3_UNORM_SRGB || im.Format == PT_FORMAT_BC5_UNORM) ? 16 : 8;
    auto mip_bytes = [&](size_t w, size_t h) { return block ? mul(mul((w + 3) / 4, (h + 3) / 4), blockBytes) : mul(mul(w, h), 4); };
    if (!((flags & 0x20000u) && mips > 0)) mips = 1;
    uint32_t maxMips = 0;
    for (uint32_t s = width > height ? width : height; s; s >>= 1) maxMips++;
    if (mips > maxMips) throw std::runtime_error("DDS: more mips than the texture size allows");
    const Bytes texels = d.from(off);
    size_t total = 0;
    for (uint32_t m = 0; m < mips; m++) {
        const size_t w = (width >> m) ? (width >> m) : 1, h = (height >> m) ? (height >> m) : 1;
        total = add(total, mip_bytes(w, h));
        if (total > texels.size) throw std::runtime_error("DDS: the header asks for more texels than the file holds");
    }
    texels.sub(0, mip_bytes(width, height)).append_to(im.Data);            // the further mips are skipped
    return im;
}

// ------------------------------------------------------------------------------------------------
// SimpleMath / DirectXMath conventions (row vectors: v' = v M), in double like ingest.py
// ------------------------------------------------------------------------------------------------
struct M4 { double m[4][4]; };
inline M4 identity() { M4 r{}; for (int i = 0; i < 4; i++) r.m[i][i] = 1.0; return r; }
inline M4 mul(const M4& a, const M4& b)
{
    M4 r{};
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { double s = 0.0; for (int k = 0; k < 4; k++) s += a.m[i][k] * b.m[k][j]; r.m[i][j] = s; }
    return r;
}
inline M4 transpose(const M4& a) { M4 r{}; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.m[i][j] = a.m[j][i]; return r; }
inline M4 rot_x(double a) { const double c = std::cos(a), s = std::sin(a); M4 r = identity(); r.m[1][1] = c; r.m[1][2] = s; r.m[2][1] = -s; r.m[2][2] = c; return r; }
inline M4 rot_y(double a) { const double c = std::cos(a), s = std::sin(a); M4 r = identity(); r.m[0][0] = c; r.m[0][2] = -s; r.m[2][0] = s; r.m[2][2] = c; return r; }
inline M4 rot_z(double a) { const double c = std::cos(a), s = std::sin(a); M4 r = identity(); r.m[0][0] = c; r.m[0][1] = s; r.m[1][0] = -s; r.m[1][1] = c; return r; }
inline M4 matrix_from_quaternion(double x, double y, double z, double w)
{
    M4 r = identity();
    r.m[0][0] = 1 - 2 * (y * y + z * z); r.m[0][1] = 2 * (x * y + z * w); r.m[0][2] = 2 * (x * z - y * w);
    r.m[1][0] = 2 * (x * y - z * w); r.m[1][1] = 1 - 2 * (x * x + z * z); r.m[1][2] = 2 * (y * z + x * w);
    r.m[2][0] = 2 * (x * z + y * w); r.m[2][1] = 2 * (y * z - x * w); r.m[2][2] = 1 - 2 * (x * x + y * y);
    return r;
}
inline double radians(double deg) { return deg * (M_PI / 180.0); }

// JSONConverters.ixx:18-26: {Yaw,Pitch,Roll} in degrees -> CreateFromYawPitchRoll(yaw, -pitch, -roll) (roll about Z first, then pitch about X,
// then yaw about Y); all three zero -> raw quaternion {X,Y,Z,W} (default identity)
inline M4 rotation_from_json(const Json* j)
{
    if (!j || j->kind != Json::Object) return identity();
    const double yaw = j->number("Yaw", 0), pitch = j->number("Pitch", 0), roll = j->number("Roll", 0);
    if (yaw == 0 && pitch == 0 && roll == 0) {
        double q[4] = { j->number("X", 0), j->number("Y", 0), j->number("Z", 0), j->number("W", 1) };
        double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (n == 0.0) n = 1.0;
        return matrix_from_quaternion(q[0] / n, q[1] / n, q[2] / n, q[3] / n);
    }
    return mul(mul(rot_z(radians(-roll)), rot_x(radians(-pitch))), rot_y(radians(yaw)));
}
inline void vec3_from_json(const Json* j, const double def[3], double out[3])
{
    out[0] = def[0]; out[1] = def[1]; out[2] = def[2];
    if (j && j->kind == Json::Object) { out[0] = j->number("X", def[0]); out[1] = j->number("Y", def[1]); out[2] = j->number("Z", def[2]); }
}
// Math::AffineTransform::operator(): Scale * Rotation * Translation (row-vector)
inline M4 affine_from_json(const Json* j)
{
    const double one[3] = { 1, 1, 1 }, zero[3] = { 0, 0, 0 };
    double s[3], t[3];
    vec3_from_json(j ? j->find("Scale") : nullptr, one, s); vec3_from_json(j ? j->find("Translation") : nullptr, zero, t);
    M4 sc = identity(); sc.m[0][0] = s[0]; sc.m[1][1] = s[1]; sc.m[2][2] = s[2];
    M4 m = mul(sc, rotation_from_json(j ? j->find("Rotation") : nullptr));
    M4 tr = identity(); tr.m[3][0] = t[0]; tr.m[3][1] = t[1]; tr.m[3][2] = t[2];
    return mul(m, tr);
}
// XMStoreFloat3x4: the column-vector affine [R|t] = top 3 rows of the transpose
inline void store_float3x4(const M4& rowMajor, float out[12]) { for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) out[4 * i + j] = (float)rowMajor.m[j][i]; }

// ------------------------------------------------------------------------------------------------
// vertex packing (VertexPositionNormalTangentTexture, Source/Vertex.ixx:38-50)
// ------------------------------------------------------------------------------------------------
struct Vertex { float Position[3]; int16_t Normal[3], Tangent[3]; uint16_t TexCoord[2][2]; };
static_assert(sizeof(Vertex) == 32, "layout");

inline int16_t encode_snorm16(double v)
{
    v = std::fmin(std::fmax(v, -1.0), 1.0) * 32767.0;
    return (int16_t)(v >= 0 ? std::floor(v + 0.5) : std::ceil(v - 0.5));
}
inline uint16_t f32_to_f16(float f)                                      // round to nearest even, like numpy's astype(float16)
{
    uint32_t x; std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);              // NaN
    if (a >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);             // >= 65536: infinity
    if (a < 0x38800000u) {                                               // below 2^-14: a subnormal half (or zero) = round(|f| * 2^24)
        float af; std::memcpy(&af, &a, 4);
        return (uint16_t)(sign | (uint32_t)std::nearbyintf(af * 16777216.0f));     // exact scaling; nearbyint rounds to nearest even
    }
    const uint32_t mant = a & 0x7FFFFFu, rem = mant & 0x1FFFu;
    uint32_t h = (((a >> 23) - 112u) << 10) | (mant >> 13);              // exponent rebias 127 -> 15
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;              // a carry runs into the exponent, up to infinity: still the right code
    return (uint16_t)(sign | h);
}

// ------------------------------------------------------------------------------------------------
// model: glTF 2.0 (.gltf with data: / external buffers, .glb)
// ------------------------------------------------------------------------------------------------
struct SkeletalVertex { float Position[3]; int16_t Normal[3], Tangent[3]; uint16_t Joints[4]; float Weights[4]; };   // VertexPositionNormalTangentSkin, Source/Vertex.ixx:52-57
static_assert(sizeof(SkeletalVertex) == 48, "layout");
// the joints of a skin: the names of their nodes and their inverse bind matrices (Model.ixx SkinJoint), shared by the mesh nodes that name the skin
struct SkinJoints { std::vector<std::string> Names; std::vector<std::array<float, 16>> InverseBindMatrices; };

struct MeshData {
    std::vector<SkeletalVertex> SkeletalVertices;                           // JOINTS_0 + WEIGHTS_0: Mesh::SkeletalVertices, with a motion-vector buffer of as many entries
    std::vector<Vertex> Vertices;
    std::vector<uint8_t> Indices; uint32_t IndexStride = 2, IndexCount = 0;      // u16 iff count <= 65535 (GLTFHelpers.ixx:183-188)
    bool HasNormals = false, HasTangents = false, HasUV[2] = { false, false };
    bool HasMaterial = false; PtMaterial Material{};
    // texture slots in the order of Material.ixx:22-33 (BaseColor, EmissiveColor, Metallic, Roughness, MetallicRoughness, Transmission, Normal);
    // textures are shared between the meshes of a model by (image, sRGB) like the reference's and the harness's loaders share them
    std::shared_ptr<struct Texture> Textures[7]; uint32_t TextureCoordinateIndex[7] = { 0, 0, 0, 0, 0, 0, 0 };
    std::vector<std::string> SkippedTextures;                               // slots whose image this host cannot load (anything but 8-bit PNG and BC1 / BC3 / BC4 / BC5 / RGBA8 DDS)
};
// base-colour / emissive textures are created as *_UNORM_SRGB (GLTFHelpers.ixx:375-391). A block-compressed DDS texture keeps the blocks
// of its file (Blocks; Texels then carries the size only) and BlockFormat names its PtFormat: the library samples them in place.
struct Texture {
    Image Texels; bool SRGB = false;
    std::vector<uint8_t> Blocks; uint32_t BlockFormat = 0;
    bool IsBlockCompressed() const { return BlockFormat != 0; }
    uint32_t Format() const { return IsBlockCompressed() ? BlockFormat : SRGB ? (uint32_t)PT_FORMAT_R8G8B8A8_UNORM_SRGB : (uint32_t)PT_FORMAT_R8G8B8A8_UNORM; }
};
enum TextureSlot { BaseColor = 0, EmissiveColor, Metallic, Roughness, MetallicRoughness, Transmission, Normal };
struct MeshNode { std::vector<MeshData> Meshes; M4 GlobalTransform;           // GlobalTransform reinterpreted as a row-vector matrix (LoadModel)
                  std::string NodeName; std::shared_ptr<SkinJoints> Skin; };  // NodeName: what an animation's transforms are looked up by; Skin: null without one

inline PtMaterial default_material()
{
    PtMaterial m{};                                                            // Material() defaults, Source/Material.ixx:13-19
    m.BaseColor[3] = 1; m.EmissiveStrength = 1; m.Roughness = 0.5f; m.IOR = 1.5f; m.AlphaCutoff = 0.5f;
    return m;
}

class Asset {
public:
    explicit Asset(const std::string& path) : dir(dir_of(path)), raw(read_file(path))
    {
        const Bytes file(raw);
        if (file.size < 12 || !file.starts_with("glTF", 4)) { j = JsonParser(file).parse(); return; }
        const Bytes glb = file.sub(0, file.le32(8), "GLB: the length in the header");
        if (glb.size < 12) throw std::runtime_error("GLB: the length in the header is shorter than the header");
        for (size_t off = 12; off < glb.size;) {                            // chunk length, chunk type, chunk
            const Bytes chunk = glb.from(off + 8).sub(0, glb.le32(off), "GLB: a chunk");
            const uint32_t ctype = glb.le32(off + 4);
            if (ctype == 0x4E4F534Au) j = JsonParser(chunk).parse();
            else if (ctype == 0x004E4942u) { binChunk = chunk; haveBin = true; }
            off += 8 + chunk.size;
        }
    }
    Json j;

    Bytes buffer(size_t i)
    {
        auto it = buffers.find(i);
        if (it != buffers.end()) return it->second;
        const Json& b = j.at("buffers").at(i);
        if (!b.has("uri")) { if (!haveBin) throw std::runtime_error("glTF: buffer without uri and no BIN chunk"); return buffers[i] = binChunk; }
        return buffers[i] = owned.emplace_back(read_uri(dir, b.at("uri").string()));
    }
    // the bytes of a bufferView: inside its buffer
    Bytes view(const Json& v, const char* what)
    {
        const Bytes b = buffer(v.at("buffer").index(j.at("buffers").size()));
        return b.sub(v.uint("byteOffset", 0, b.size), v.at("byteLength").uint(b.size), what);
    }
    // element (i, c) of an accessor as double (integers as they are; normalised integers divided by their maximum, in float like ingest.py)
    struct Accessor { const uint8_t* data; size_t stride, count; int ncomp, ctype; bool normalized; };
    // validated here, once: [data, data + (count - 1) * stride + element size) lies inside the accessor's bufferView
    Accessor accessor(const Json& index)
    {
        const Json& a = j.at("accessors").pick(index);
        const Json& v = j.at("bufferViews").pick(a.at("bufferView"));
        const Bytes b = view(v, "glTF: the bufferView of an accessor");
        Accessor r;
        r.ctype = (int)a.at("componentType").uint(0xFFFF);
        const std::string& t = a.at("type").string();
        r.ncomp = t == "SCALAR" ? 1 : t == "VEC2" ? 2 : t == "VEC3" ? 3 : t == "VEC4" ? 4 : t == "MAT4" ? 16 : 0;
        if (!r.ncomp) throw std::runtime_error("glTF: accessor type " + t);
        const size_t elem = (size_t)component_size(r.ctype) * r.ncomp, vstride = v.uint("byteStride", 0, 252);     // (252: glTF's limit)
        r.stride = (vstride == 0 || vstride == elem) ? elem : vstride;
        r.count = a.at("count").uint(b.size);                             // (an element has at least one byte)
        const size_t extent = r.count ? add(mul(r.count - 1, r.stride), elem) : 0;
        r.data = b.sub(a.uint("byteOffset", 0, b.size), extent, "glTF: an accessor in its bufferView").data;
        const Json* n = a.find("normalized");
        r.normalized = n && n->kind == Json::Bool && n->b;
        return r;
    }
    static int component_size(int ctype)
    {
        switch (ctype) { case 5120: case 5121: return 1; case 5122: case 5123: return 2; case 5125: case 5126: return 4; }
        throw std::runtime_error("glTF: component type " + std::to_string(ctype));
    }
    static double element(const Accessor& a, size_t i, int c)
    {
        const uint8_t* p = a.data + i * a.stride + (size_t)c * component_size(a.ctype);
        double v; float maxv = 1.0f;
        switch (a.ctype) {
        case 5120: { int8_t x; std::memcpy(&x, p, 1); v = x; maxv = 127.0f; break; }
        case 5121: { uint8_t x; std::memcpy(&x, p, 1); v = x; maxv = 255.0f; break; }
        case 5122: { int16_t x; std::memcpy(&x, p, 2); v = x; maxv = 32767.0f; break; }
        case 5123: { uint16_t x; std::memcpy(&x, p, 2); v = x; maxv = 65535.0f; break; }
        case 5125: { uint32_t x; std::memcpy(&x, p, 4); v = x; maxv = 4294967295.0f; break; }
        default: { float x; std::memcpy(&x, p, 4); return x; }
        }
        return a.normalized ? (double)((float)v / maxv) : v;
    }

    const Json& image(const Json& index) const { return j.at("images").pick(index); }
    // the encoded bytes of an image: a view of its bufferView, or of hold, which receives what a data: / file uri names
    Bytes image_bytes(const Json& im, std::string& hold)
    {
        if (im.has("uri")) return hold = read_uri(dir, im.at("uri").string());
        return view(j.at("bufferViews").pick(im.at("bufferView")), "glTF: the bufferView of an image");
    }

    // a DDS image by its mime type, its file name or its first four bytes
    static bool image_is_dds(const Json& im, Bytes bytes)
    {
        if (im.has("mimeType") && im.at("mimeType").string() == "image/vnd-ms.dds") return true;
        if (im.has("uri")) {
            const std::string& uri = im.at("uri").string();
            if (uri.compare(0, 5, "data:") && uri.size() >= 4) {
                std::string tail(uri.end() - 4, uri.end());
                for (char& c : tail) c = (char)std::tolower((unsigned char)c);
                if (tail == ".dds") return true;
            }
        }
        return is_dds(bytes);
    }

private:
    const std::string dir, raw;                                             // raw: the file; the BIN chunk and the views into it point here
    Bytes binChunk; bool haveBin = false;
    std::map<size_t, Bytes> buffers; std::deque<std::string> owned;         // owned: buffers that a uri names (a deque never moves them)
};

// [DirectXMesh spec] ComputeTangentFrame (tangent output only): same operations in the same order as ingest.py's compute_tangents
inline std::vector<std::array<double, 3>> compute_tangents(const std::vector<std::array<float, 3>>& pos, const std::vector<std::array<float, 3>>& nrm,
                                                           const std::vector<std::array<float, 2>>& uv, const std::vector<uint32_t>& idx)
{
    std::vector<std::array<double, 3>> tan(pos.size(), { 0.0, 0.0, 0.0 });
    for (size_t t = 0; t + 2 < idx.size(); t += 3) {
        const uint32_t a = idx[t], b = idx[t + 1], c = idx[t + 2];
        double e1[3], e2[3];
        for (int k = 0; k < 3; k++) { e1[k] = (double)pos[b][k] - (double)pos[a][k]; e2[k] = (double)pos[c][k] - (double)pos[a][k]; }
        const double du1 = (double)uv[b][0] - (double)uv[a][0], dv1 = (double)uv[b][1] - (double)uv[a][1];
        const double du2 = (double)uv[c][0] - (double)uv[a][0], dv2 = (double)uv[c][1] - (double)uv[a][1];
        const double det = du1 * dv2 - du2 * dv1;
        if (std::fabs(det) < 1e-20) continue;
        for (int k = 0; k < 3; k++) { const double s = (e1[k] * dv2 - e2[k] * dv1) / det; tan[a][k] += s; tan[b][k] += s; tan[c][k] += s; }
    }
    for (size_t i = 0; i < pos.size(); i++) {
        const double n[3] = { nrm[i][0], nrm[i][1], nrm[i][2] };
        const double d = (n[0] * tan[i][0] + n[1] * tan[i][1]) + n[2] * tan[i][2];
        double t[3] = { tan[i][0] - n[0] * d, tan[i][1] - n[1] * d, tan[i][2] - n[2] * d };
        const double ln = std::sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
        double f[3] = { n[1] * 0.0 - n[2] * 1.0, n[2] * 0.0 - n[0] * 0.0, n[0] * 1.0 - n[1] * 0.0 };   // cross(n, (0, 1, 0))
        const double fl = std::sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
        if (fl > 1e-8) { const double dd = std::fmax(fl, 1e-30); f[0] /= dd; f[1] /= dd; f[2] /= dd; } else { f[0] = 1.0; f[1] = 0.0; f[2] = 0.0; }
        if (ln > 1e-12) { const double dd = std::fmax(ln, 1e-30); tan[i] = { t[0] / dd, t[1] / dd, t[2] / dd }; } else tan[i] = { f[0], f[1], f[2] };
    }
    return tan;
}

// glTF column-vector local matrix of a node
inline M4 node_matrix(const Json& node)
{
    if (node.has("matrix")) { M4 c{}; const Json& m = node.at("matrix"); for (int i = 0; i < 16; i++) c.m[i / 4][i % 4] = m.at((size_t)i).real(); return transpose(c); }   // column-major list
    M4 t = identity(), r = identity(), s = identity();
    if (node.has("translation")) for (int k = 0; k < 3; k++) t.m[k][3] = node.at("translation").at((size_t)k).real();
    if (node.has("rotation")) { const Json& q = node.at("rotation"); r = transpose(matrix_from_quaternion(q.at(0).real(), q.at(1).real(), q.at(2).real(), q.at(3).real())); }
    if (node.has("scale")) for (int k = 0; k < 3; k++) s.m[k][k] = node.at("scale").at((size_t)k).real();
    return mul(mul(t, r), s);
}

// GLTFHelpers::LoadModel: one MeshNode per glTF node that carries a mesh, with its global transform
inline std::vector<std::shared_ptr<MeshNode>> load_model(const std::string& path, bool flipWindingOrder = true)
{
    Asset asset(path);
    const Json& j = asset.j;
    std::map<std::pair<const Json*, bool>, std::shared_ptr<Texture>> textureCache;          // (image, forced sRGB) -> texture; nullptr: not decodable here
    auto texture_for = [&](const Json& info, bool forceSrgb) -> std::shared_ptr<Texture> {
        const Json& tex = j.at("textures").pick(info.at("index"));
        const Json* ext = tex.find("extensions");
        const Json* msft = ext ? ext->find("MSFT_texture_dds") : nullptr;                // the DDS image wins over the PNG (GLTFHelpers.ixx:87-90,103,451)
        const Json& im = asset.image(msft && msft->has("source") ? msft->at("source") : tex.at("source"));
        const auto key = std::make_pair(&im, forceSrgb);
        auto it = textureCache.find(key);
        if (it != textureCache.end()) return it->second;
        std::shared_ptr<Texture> t;
        std::string hold;
        const Bytes bytes = asset.image_bytes(im, hold);
        if (Asset::image_is_dds(im, bytes)) {                              // forceSRGB: a UNORM DDS in these slots gets the _SRGB format (TextureHelpers.ixx:68)
            try {
                DdsImage dds = read_dds(bytes);
                if (forceSrgb) dds.Format = dds.Format == PT_FORMAT_R8G8B8A8_UNORM ? (uint32_t)PT_FORMAT_R8G8B8A8_UNORM_SRGB : dds.Format == PT_FORMAT_BC1_UNORM ? (uint32_t)PT_FORMAT_BC1_UNORM_SRGB
                                       : dds.Format == PT_FORMAT_BC3_UNORM ? (uint32_t)PT_FORMAT_BC3_UNORM_SRGB : dds.Format;
                t = std::make_shared<Texture>(); t->Texels.Width = dds.Width; t->Texels.Height = dds.Height;
                if (dds.Format >= PT_FORMAT_BC1_UNORM) { t->Blocks = std::move(dds.Data); t->BlockFormat = dds.Format; }
                else { t->Texels.RGBA = std::move(dds.Data); }
                t->SRGB = dds.Format == PT_FORMAT_R8G8B8A8_UNORM_SRGB || dds.Format == PT_FORMAT_BC1_UNORM_SRGB || dds.Format == PT_FORMAT_BC3_UNORM_SRGB;
            } catch (const std::exception&) { t.reset(); }
        } else if (is_png(bytes)) { try { t = std::make_shared<Texture>(); t->Texels = decode_png(bytes); t->SRGB = forceSrgb; } catch (const std::exception&) { t.reset(); } }
        return textureCache[key] = t;
    };
    auto process_primitive = [&](const Json& prim, MeshData& mesh) -> bool {
        if (prim.uint("mode", 4, 0xFFFF) != 4 || !prim.has("attributes") || !prim.at("attributes").has("POSITION") || !prim.has("indices")) return false;   // :150-152,169-171,191-193
        const Json& attrs = prim.at("attributes");
        const Asset::Accessor pa = asset.accessor(attrs.at("POSITION"));
        if (pa.ncomp < 3) throw std::runtime_error("glTF: POSITION is not a VEC3");
        std::vector<std::array<float, 3>> pos(pa.count);
        for (size_t i = 0; i < pa.count; i++) for (int k = 0; k < 3; k++) pos[i][k] = (float)Asset::element(pa, i, k);
        const Asset::Accessor ia = asset.accessor(prim.at("indices"));
        if (ia.ctype != 5121 && ia.ctype != 5123 && ia.ctype != 5125) throw std::runtime_error("glTF: indices are not unsigned integers");   // (so the conversion below is exact)
        std::vector<uint32_t> idx(ia.count);
        for (size_t i = 0; i < ia.count; i++) { idx[i] = (uint32_t)Asset::element(ia, i, 0); if (idx[i] >= pa.count) throw std::runtime_error("glTF: vertex index beyond the POSITION accessor"); }
        if (flipWindingOrder) for (size_t i = 0; i < idx.size() / 2; i++) std::swap(idx[i], idx[idx.size() - 1 - i]);        // slot count-1-i <- index i (:179)
        std::vector<std::array<float, 2>> uv[2];
        for (int s = 0; s < 2; s++) {
            const std::string name = "TEXCOORD_" + std::to_string(s);
            if (!attrs.has(name)) continue;
            const Asset::Accessor ua = asset.accessor(attrs.at(name));
            if (ua.count != pa.count || ua.ncomp < 2) throw std::runtime_error("glTF: " + name + " does not match POSITION");
            uv[s].resize(ua.count);
            for (size_t i = 0; i < ua.count; i++) for (int k = 0; k < 2; k++) uv[s][i][k] = (float)Asset::element(ua, i, k);
            mesh.HasUV[s] = true;
        }
        std::vector<std::array<float, 3>> nrm; std::vector<std::array<double, 3>> tan;
        if (attrs.has("NORMAL")) {
            const Asset::Accessor na = asset.accessor(attrs.at("NORMAL"));
            if (na.count != pa.count || na.ncomp < 3) throw std::runtime_error("glTF: NORMAL does not match POSITION");
            nrm.resize(na.count);
            for (size_t i = 0; i < na.count; i++) for (int k = 0; k < 3; k++) nrm[i][k] = (float)Asset::element(na, i, k);
            mesh.HasNormals = true;
            if (mesh.HasUV[0]) { tan = compute_tangents(pos, nrm, uv[0], idx); mesh.HasTangents = true; }     // "Tangent" is never found -> always recomputed (:251-275)
        }
        mesh.Vertices.assign(pos.size(), Vertex{});
        for (size_t i = 0; i < pos.size(); i++) {
            Vertex& v = mesh.Vertices[i];
            for (int k = 0; k < 3; k++) {
                v.Position[k] = pos[i][k];
                if (mesh.HasNormals) v.Normal[k] = encode_snorm16((double)nrm[i][k]);
                if (mesh.HasTangents) v.Tangent[k] = encode_snorm16(tan[i][k]);
            }
            for (int s = 0; s < 2; s++) if (mesh.HasUV[s]) for (int k = 0; k < 2; k++) v.TexCoord[s][k] = f32_to_f16(uv[s][i][k]);
        }
        mesh.IndexCount = (uint32_t)idx.size(); mesh.IndexStride = idx.size() <= 65535 ? 2u : 4u;
        mesh.Indices.resize((size_t)mesh.IndexCount * mesh.IndexStride);
        for (size_t i = 0; i < idx.size(); i++) {
            if (mesh.IndexStride == 2) { const uint16_t x = (uint16_t)idx[i]; std::memcpy(mesh.Indices.data() + 2 * i, &x, 2); }
            else std::memcpy(mesh.Indices.data() + 4 * i, &idx[i], 4);
        }
        if (attrs.has("JOINTS_0") && attrs.has("WEIGHTS_0")) {           // :278-304: u8 / u16 joints become XMUSHORT4, normalised-integer weights are converted
            const Asset::Accessor ja = asset.accessor(attrs.at("JOINTS_0"));
            Asset::Accessor wa = asset.accessor(attrs.at("WEIGHTS_0"));
            if ((ja.ctype != 5121 && ja.ctype != 5123) || ja.ncomp != 4) throw std::runtime_error("glTF: JOINTS_0 is not a VEC4 of unsigned bytes or shorts");
            if (wa.ncomp != 4 || ja.count != pa.count || wa.count != pa.count) throw std::runtime_error("glTF: JOINTS_0 / WEIGHTS_0 do not match the POSITION accessor");
            if (wa.ctype != 5126) wa.normalized = true;                    // integer weights are normalised ones, flagged or not (as ingest.py)
            mesh.SkeletalVertices.assign(pos.size(), SkeletalVertex{});
            for (size_t i = 0; i < pos.size(); i++) {
                SkeletalVertex& sv = mesh.SkeletalVertices[i]; const Vertex& v = mesh.Vertices[i];
                for (int k = 0; k < 3; k++) { sv.Position[k] = v.Position[k]; sv.Normal[k] = v.Normal[k]; sv.Tangent[k] = v.Tangent[k]; }
                for (int k = 0; k < 4; k++) { sv.Joints[k] = (uint16_t)Asset::element(ja, i, k); sv.Weights[k] = (float)Asset::element(wa, i, k); }
            }
        }
        if (prim.has("material")) {
            const Json& m = j.at("materials").pick(prim.at("material"));
            static const Json empty = [] { Json e; e.kind = Json::Object; return e; }();
            const Json& pbr = m.has("pbrMetallicRoughness") ? m.at("pbrMetallicRoughness") : empty;
            const Json& ext = m.has("extensions") ? m.at("extensions") : empty;
            PtMaterial mat = default_material();
            if (pbr.has("baseColorFactor")) for (int k = 0; k < 4; k++) mat.BaseColor[k] = pbr.at("baseColorFactor").at((size_t)k).f32();
            else for (int k = 0; k < 4; k++) mat.BaseColor[k] = 1.0f;
            mat.EmissiveStrength = ext.has("KHR_materials_emissive_strength") ? ext.at("KHR_materials_emissive_strength").f32("emissiveStrength", 1.0) : 1.0f;
            for (int k = 0; k < 3; k++) mat.EmissiveColor[k] = m.has("emissiveFactor") ? m.at("emissiveFactor").at((size_t)k).f32() : 0.0f;
            mat.Metallic = pbr.f32("metallicFactor", 1.0);
            mat.Roughness = pbr.f32("roughnessFactor", 1.0);
            mat.IOR = ext.has("KHR_materials_ior") ? ext.at("KHR_materials_ior").f32("ior", 1.5) : 1.5f;
            const std::string am = m.has("alphaMode") ? m.at("alphaMode").string() : "OPAQUE";
            mat.AlphaMode = am == "MASK" ? 1u : am == "BLEND" ? 2u : 0u;
            mat.AlphaCutoff = m.f32("alphaCutoff", 0.5);
            const Json* tr = ext.find("KHR_materials_transmission");
            if (tr && tr->kind == Json::Object) mat.Transmission = tr->f32("transmissionFactor", 0.0);
            mesh.Material = mat; mesh.HasMaterial = true;
            if (mesh.HasUV[0] || mesh.HasUV[1]) {                          // :370-428
                auto slot = [&](TextureSlot k, const char* name, const Json* info, bool srgb) {
                    if (!info || info->kind != Json::Object) return;
                    const size_t tc = info->uint("texCoord", 0, UINT32_MAX);   // any set is valid glTF; this host keeps two
                    if (tc >= 2 || !mesh.HasUV[tc]) return;
                    if (auto t = texture_for(*info, srgb)) { mesh.Textures[k] = t; mesh.TextureCoordinateIndex[k] = (uint32_t)tc; }
                    else mesh.SkippedTextures.push_back(name);
                };
                slot(BaseColor, "BaseColor", pbr.find("baseColorTexture"), true); slot(EmissiveColor, "EmissiveColor", m.find("emissiveTexture"), true);
                slot(MetallicRoughness, "MetallicRoughness", pbr.find("metallicRoughnessTexture"), false);
                slot(Transmission, "Transmission", tr ? tr->find("transmissionTexture") : nullptr, false);
                if (mesh.HasTangents) slot(Normal, "Normal", m.find("normalTexture"), false);   // a normal map needs the tangent frame
            }
        }
        return true;
    };

    std::vector<std::shared_ptr<MeshNode>> out;
    std::map<size_t, std::shared_ptr<SkinJoints>> skins;
    const Json& scene = j.at("scenes").at(j.uint("scene", 0, Json::kMaxUint));
    // depth first, children in file order, on an explicit stack (a chain of nodes may be as long as the file allows). glTF wants a strict
    // tree: a node reached a second time, through a cycle or through a second parent, is refused -- shared children could repeat a subtree
    // exponentially often.
    static const std::vector<Json> none;
    const std::vector<Json>& nodes = j.has("nodes") ? j.at("nodes").items() : none;
    std::vector<bool> visited(nodes.size(), false);
    std::vector<std::pair<size_t, M4>> pending;                            // (node, its parent's global matrix)
    auto push = [&](const Json& list, const M4& parent) {
        for (size_t k = list.items().size(); k--;) pending.emplace_back(list.items()[k].index(nodes.size()), parent);
    };
    if (scene.has("nodes")) push(scene.at("nodes"), identity());
    while (!pending.empty()) {
        const auto [ni, parent] = pending.back(); pending.pop_back();
        if (visited[ni]) throw std::runtime_error("glTF: node " + std::to_string(ni) + " is reached twice (a cycle, or a second parent)");
        visited[ni] = true;
        const Json& node = nodes[ni];
        const M4 m = mul(parent, node_matrix(node));
        if (node.has("mesh")) {
            const Json& mj = j.at("meshes").pick(node.at("mesh"));
            if (mj.has("primitives") && mj.at("primitives").size()) {
                auto mn = std::make_shared<MeshNode>();
                for (const Json& p : mj.at("primitives").items()) { MeshData md; if (process_primitive(p, md)) mn->Meshes.push_back(std::move(md)); }
                mn->GlobalTransform = transpose(m);                       // the column-vector global matrix reinterpreted as a row-vector Matrix
                if (node.has("name")) mn->NodeName = node.at("name").string();
                if (node.has("skin")) {                                    // :477-512: joint names + inverse bind matrices, shared per skin index
                    const size_t si = node.at("skin").index(j.has("skins") ? j.at("skins").size() : 0);
                    if (!skins.count(si)) {
                        skins[si] = nullptr;
                        const Json& skin = j.at("skins").at(si);
                        if (skin.has("inverseBindMatrices")) {             // a skin without them is ignored (:484)
                            const Asset::Accessor ia = asset.accessor(skin.at("inverseBindMatrices"));
                            if (ia.ctype != 5126 || ia.ncomp != 16) throw std::runtime_error("glTF: inverseBindMatrices is not a MAT4 of floats");
                            auto sj = std::make_shared<SkinJoints>();
                            if (skin.has("joints")) for (const Json& jn : skin.at("joints").items()) { const Json& n = nodes[jn.index(nodes.size())]; sj->Names.push_back(n.has("name") ? n.at("name").string() : std::string()); }
                            if (ia.count > sj->Names.size()) throw std::runtime_error("glTF: more inverse bind matrices than joints");
                            sj->Names.resize(ia.count);
                            // glTF's column-major column-vector matrix, reinterpreted as a row-vector Matrix (:492): the floats as they lie
                            for (size_t k = 0; k < ia.count; k++) { std::array<float, 16> mtx; for (int e = 0; e < 16; e++) mtx[e] = (float)Asset::element(ia, k, e); sj->InverseBindMatrices.push_back(mtx); }
                            skins[si] = sj;
                        }
                    }
                    mn->Skin = skins[si];
                }
                out.push_back(mn);
            }
        }
        if (node.has("children")) push(node.at("children"), m);
    }
    return out;
}

// ------------------------------------------------------------------------------------------------
// animations: GLTFHelpers::LoadAnimation (GLTFHelpers.ixx:539-663) -> a rig as pt_anim_create_rig takes it
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kNoNode = PT_ANIM_NO_NODE;
struct Rig {
    std::vector<int32_t> Parents;                                           // depth first, parent < own index, -1 for a root
    std::vector<float> Rest;                                                // 10 per node: Translation, Rotation (x, y, z, w), Scale
    std::vector<std::string> Names, ClipNames;
    std::vector<double> Durations;                                          // per clip
    std::vector<uint32_t> Channels;                                         // [clip][node][T, R, S][FirstKey, KeyCount]
    std::vector<float> KeyTimes, KeyValues;                                 // KeyValues: 4 per key
    // m_globalTransforms.find(name): the LAST node of that name in traversal order (the reference's map entry is overwritten), or kNoNode
    uint32_t FindNode(const std::string& name) const { for (size_t n = Names.size(); n--;) if (Names[n] == name) return (uint32_t)n; return kNoNode; }
};

// fastgltf's DecomposeNodeMatrices on a column-vector matrix, the operations of ingest.py's decompose in the same order
inline void decompose(const M4& m, double t[3], double q[4], double sc[3])
{
    for (int k = 0; k < 3; k++) { t[k] = m.m[k][3]; sc[k] = std::sqrt((m.m[0][k] * m.m[0][k] + m.m[1][k] * m.m[1][k]) + m.m[2][k] * m.m[2][k]); }
    const double det = m.m[0][0] * (m.m[1][1] * m.m[2][2] - m.m[1][2] * m.m[2][1]) - m.m[0][1] * (m.m[1][0] * m.m[2][2] - m.m[1][2] * m.m[2][0])
                     + m.m[0][2] * (m.m[1][0] * m.m[2][1] - m.m[1][1] * m.m[2][0]);
    if (det < 0) sc[0] = -sc[0];
    double r[3][3];
    for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) r[i][k] = m.m[i][k] / (sc[k] == 0 ? 1.0 : sc[k]);
    const double tr = r[0][0] + r[1][1] + r[2][2];
    if (tr > 0) { const double k = std::sqrt(tr + 1.0) * 2; q[0] = (r[2][1] - r[1][2]) / k; q[1] = (r[0][2] - r[2][0]) / k; q[2] = (r[1][0] - r[0][1]) / k; q[3] = 0.25 * k; }
    else if (r[0][0] > r[1][1] && r[0][0] > r[2][2]) { const double k = std::sqrt(1.0 + r[0][0] - r[1][1] - r[2][2]) * 2; q[0] = 0.25 * k; q[1] = (r[0][1] + r[1][0]) / k; q[2] = (r[0][2] + r[2][0]) / k; q[3] = (r[2][1] - r[1][2]) / k; }
    else if (r[1][1] > r[2][2]) { const double k = std::sqrt(1.0 + r[1][1] - r[0][0] - r[2][2]) * 2; q[0] = (r[0][1] + r[1][0]) / k; q[1] = 0.25 * k; q[2] = (r[1][2] + r[2][1]) / k; q[3] = (r[0][2] - r[2][0]) / k; }
    else { const double k = std::sqrt(1.0 + r[2][2] - r[0][0] - r[1][1]) * 2; q[0] = (r[0][2] + r[2][0]) / k; q[1] = (r[1][2] + r[2][1]) / k; q[2] = 0.25 * k; q[3] = (r[1][0] - r[0][1]) / k; }
}

// The default scene's node forest, flattened depth first with its decomposed TRS, and one clip per glTF animation. LINEAR samplers only (STEP and
// CUBICSPLINE channels are skipped, :582-584), channels without a target node are skipped, and per node NAME and path the first channel wins
// (:593, :616, :639); a clip's duration is the largest key time of the channels it accepted.
// The reference keeps keyframes and global transforms in maps keyed by node name. Names are resolved to indices HERE, with the maps' semantics:
// the keyframes of a name apply to every node of the forest that carries it (Animation.ixx:123), and a lookup BY name (Rig::FindNode: a mesh
// node, a joint) finds the LAST node of that name in traversal order, because m_globalTransforms[name] is overwritten (:138).
inline std::shared_ptr<Rig> load_animation(const std::string& path)
{
    Asset asset(path);
    const Json& j = asset.j;
    auto rig = std::make_shared<Rig>();
    static const std::vector<Json> none;
    const std::vector<Json>& nodes = j.has("nodes") ? j.at("nodes").items() : none;
    const Json& scene = j.at("scenes").at(j.uint("scene", 0, Json::kMaxUint));
    auto name_of = [&](const Json& n) { return n.has("name") ? n.at("name").string() : std::string(); };
    std::vector<bool> visited(nodes.size(), false);
    std::vector<std::pair<size_t, int32_t>> pending;                       // (node, its parent's index in the rig)
    auto push = [&](const Json& list, int32_t parent) { for (size_t k = list.items().size(); k--;) pending.emplace_back(list.items()[k].index(nodes.size()), parent); };
    if (scene.has("nodes")) push(scene.at("nodes"), -1);
    while (!pending.empty()) {
        const auto [ni, parent] = pending.back(); pending.pop_back();
        if (visited[ni]) throw std::runtime_error("glTF: node " + std::to_string(ni) + " is reached twice (a cycle, or a second parent)");
        visited[ni] = true;
        const Json& node = nodes[ni];
        double t[3] = { 0, 0, 0 }, q[4] = { 0, 0, 0, 1 }, sc[3] = { 1, 1, 1 };
        if (node.has("matrix")) decompose(node_matrix(node), t, q, sc);
        else {
            auto read = [&](const char* key, double* dst, size_t n) { if (!node.has(key)) return; if (node.at(key).items().size() != n) throw std::runtime_error(std::string("glTF: a node's ") + key + " of the wrong length"); for (size_t k = 0; k < n; k++) dst[k] = node.at(key).at(k).real(); };
            read("translation", t, 3); read("rotation", q, 4); read("scale", sc, 3);
        }
        const int32_t me = (int32_t)rig->Parents.size();
        rig->Parents.push_back(parent); rig->Names.push_back(name_of(node));
        for (double v : t) rig->Rest.push_back((float)v);
        for (double v : q) rig->Rest.push_back((float)v);
        for (double v : sc) rig->Rest.push_back((float)v);
        if (node.has("children")) push(node.at("children"), me);
    }
    const size_t n = rig->Parents.size();
    if (!j.has("animations") || !j.at("animations").size()) throw std::runtime_error(path + ": the file holds no animation");
    const std::vector<Json>& anims = j.at("animations").items();
    rig->Channels.assign(mul(mul(anims.size(), n), 6), 0u);
    for (size_t ci = 0; ci < anims.size(); ci++) {
        const Json& anim = anims[ci];
        float duration = 0.0f;
        std::map<std::pair<std::string, int>, std::pair<uint32_t, uint32_t>> taken;      // (node name, path) -> (FirstKey, KeyCount): the first channel wins
        if (anim.has("channels")) for (const Json& ch : anim.at("channels").items()) {
            const Json* target = ch.find("target");
            if (!target || !target->has("node")) continue;
            const Json& sampler = anim.at("samplers").pick(ch.at("sampler"));
            if (sampler.has("interpolation") && sampler.at("interpolation").string() != "LINEAR") continue;
            const std::string pathName = target->has("path") ? target->at("path").string() : std::string();
            const int slot = pathName == "translation" ? 0 : pathName == "rotation" ? 1 : pathName == "scale" ? 2 : -1;
            if (slot < 0) continue;                                        // weights: morph targets are out of scope
            const size_t ncomp = slot == 1 ? 4 : 3;
            const std::string name = name_of(nodes[target->at("node").index(nodes.size())]);
            if (taken.count({ name, slot })) continue;
            const Asset::Accessor ta = asset.accessor(sampler.at("input")), va = asset.accessor(sampler.at("output"));
            if (ta.ctype != 5126 || ta.ncomp != 1) throw std::runtime_error("glTF: an animation sampler's input is not a SCALAR of floats");
            if ((size_t)va.ncomp != ncomp || va.ctype != 5126) throw std::runtime_error("glTF: an animation sampler's output does not fit the " + pathName + " path");
            if (ta.count != va.count) throw std::runtime_error("glTF: an animation sampler's input and output counts differ");
            if (!ta.count) continue;                                       // an empty channel leaves the slot empty: a later one may take it
            if (add(rig->KeyTimes.size(), ta.count) > UINT32_MAX) throw std::runtime_error("glTF: more than 2^32 keys");
            const uint32_t first = (uint32_t)rig->KeyTimes.size();
            for (size_t k = 0; k < ta.count; k++) {
                const float time = (float)Asset::element(ta, k, 0);
                bool ok = std::isfinite(time) && (k == 0 || time > rig->KeyTimes.back());
                rig->KeyTimes.push_back(time);
                for (size_t c = 0; c < 4; c++) { const float v = c < ncomp ? (float)Asset::element(va, k, (int)c) : 0.0f; ok = ok && std::isfinite(v); rig->KeyValues.push_back(v); }
                if (!ok) throw std::runtime_error("glTF: key times must be finite and strictly ascending, key values finite");
                duration = std::fmax(duration, time);
            }
            taken[{ name, slot }] = { first, (uint32_t)ta.count };
        }
        for (size_t ni = 0; ni < n; ni++) for (int slot = 0; slot < 3; slot++) {       // the keyframes of a name apply to every node that carries it
            auto it = taken.find({ rig->Names[ni], slot });
            if (it == taken.end()) continue;
            uint32_t* c = rig->Channels.data() + ((ci * n + ni) * 3 + (size_t)slot) * 2;
            c[0] = it->second.first; c[1] = it->second.second;
        }
        rig->Durations.push_back((double)duration);
        rig->ClipNames.push_back(anim.has("name") ? anim.at("name").string() : std::string());
    }
    return rig;
}

// ------------------------------------------------------------------------------------------------
// scene descriptor + Scene::Load / Refresh
// ------------------------------------------------------------------------------------------------
// a render object with an animation bound (Scene.ixx:165-168), as pt_anim_create_object takes it
struct AnimatedObject {
    std::shared_ptr<Rig> Animation;
    float Transform[16];                                                    // RenderObject.Transform(), row-vector convention
    std::vector<uint32_t> BindingNodes, BindingInstances; std::vector<float> BindingGlobals;   // per mesh node: rig node (or kNoNode), instance, GlobalTransform
    struct Skin { uint32_t MeshNode; std::vector<uint32_t> JointNodes; std::vector<float> InverseBinds; uint32_t SceneNode; };
    std::vector<Skin> Skins;                                                // per skinned mesh node; SceneNode: index into Scene::Nodes
};
struct RenderObject { uint32_t Node; float Transform[12]; bool IsVisible; std::string Name; };   // Transform: column-vector [R|t], as InstanceData.ObjectToWorld wants it
struct Scene {
    double CameraPosition[3] = { 0, 0, 0 }; M4 CameraRotation = identity();
    float EnvironmentLightColor[4] = { 0, 0, 0, -1 }; float EnvironmentLightTransform[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    std::string EnvironmentLightTexture;                                    // path, not decoded here
    std::vector<std::shared_ptr<MeshNode>> Nodes;                           // one bottom level each
    std::vector<RenderObject> Objects;                                      // one instance each
    std::vector<AnimatedObject> Animations;                                 // one per render object that names an animation
};

inline Scene load_scene(const std::string& path)
{
    const Json j = JsonParser(read_file(path)).parse();
    const std::string base = dir_of(path);
    Scene sc;
    const double zero[3] = { 0, 0, 0 };
    const Json* cam = j.find("Camera");
    vec3_from_json(cam ? cam->find("Position") : nullptr, zero, sc.CameraPosition);
    sc.CameraRotation = rotation_from_json(cam ? cam->find("Rotation") : nullptr);
    const Json* env = j.find("EnvironmentLight");
    if (env && env->kind == Json::Object) {
        if (const Json* col = env->find("Color"); col && col->kind == Json::Object) {
            sc.EnvironmentLightColor[0] = col->f32("R", 0); sc.EnvironmentLightColor[1] = col->f32("G", 0);
            sc.EnvironmentLightColor[2] = col->f32("B", 0); sc.EnvironmentLightColor[3] = col->f32("A", -1);
        } else sc.EnvironmentLightColor[3] = -1;
        store_float3x4(rotation_from_json(env->find("Rotation")), sc.EnvironmentLightTransform);     // App.cpp:1019
        if (env->has("Texture")) sc.EnvironmentLightTexture = resolve(base, env->at("Texture").string());
    }
    std::map<std::string, std::string> models;
    if (const Json* m = j.find("Models"); m && m->kind == Json::Object) for (auto& kv : m->obj) models[kv.first] = resolve(base, kv.second.string());
    std::map<std::string, std::string> animations;
    if (const Json* m = j.find("Animations"); m && m->kind == Json::Object) for (auto& kv : m->obj) animations[kv.first] = resolve(base, kv.second.string());
    std::map<std::string, std::shared_ptr<Rig>> rigs;
    std::map<std::string, std::vector<std::shared_ptr<MeshNode>>> loaded;
    M4 zflip = identity(); zflip.m[2][2] = -1.0;
    if (const Json* ros = j.find("RenderObjects"); ros && ros->kind == Json::Array)
        for (const Json& ro : ros->arr) {
            const std::string model = ro.has("Model") ? ro.at("Model").string() : "", name = ro.has("Name") ? ro.at("Name").string() : "";
            if (!model.empty() && !models.count(model))                    // MyScene.ixx:57-70
                throw std::runtime_error(path + ": " + (name.empty() ? std::string("Unnamed RenderObject") : "RenderObject " + name) + ": Models " + model + " not found");
            const std::string animation = ro.has("Animation") ? ro.at("Animation").string() : "";
            if (!animation.empty() && !animations.count(animation))        // MyScene.ixx:69
                throw std::runtime_error(path + ": " + (name.empty() ? std::string("Unnamed RenderObject") : "RenderObject " + name) + ": Animations " + animation + " not found");
            if (model.empty()) continue;
            if (!loaded.count(model)) loaded[model] = load_model(models[model], true);      // Scene.ixx:90
            const M4 transform = affine_from_json(ro.find("Transform"));
            const Json* vis = ro.find("IsVisible");
            std::shared_ptr<Rig> rig;
            if (!animation.empty()) { if (!rigs.count(animation)) rigs[animation] = load_animation(animations[animation]); rig = rigs[animation]; }
            AnimatedObject ao; ao.Animation = rig;
            for (int e = 0; e < 16; e++) ao.Transform[e] = (float)transform.m[e / 4][e % 4];
            // Model.SkinJoints is a dictionary keyed by the mesh node's name: the last skin stored under a name serves every mesh node of that name
            std::map<std::string, std::shared_ptr<SkinJoints>> skinOf;
            for (auto& mn : loaded[model]) if (mn->Skin) skinOf[mn->NodeName] = mn->Skin;
            for (auto mn : loaded[model]) {
                bool skinned = false;
                for (const MeshData& md : mn->Meshes) skinned = skinned || !md.SkeletalVertices.empty();
                // the skinning pass rewrites the vertex buffer in place: a skinned mesh node is instanced once per animated render object
                if (rig && skinned) mn = std::make_shared<MeshNode>(*mn);
                uint32_t ni = 0;
                for (; ni < sc.Nodes.size(); ni++) if (sc.Nodes[ni] == mn) break;
                if (ni == sc.Nodes.size()) sc.Nodes.push_back(mn);
                RenderObject o; o.Node = ni; o.Name = name; o.IsVisible = !(vis && vis->kind == Json::Bool && !vis->b);
                store_float3x4(mul(mul(mn->GlobalTransform, zflip), transform), o.Transform);     // Scene.ixx:199-214
                if (rig) {
                    ao.BindingNodes.push_back(rig->FindNode(mn->NodeName)); ao.BindingInstances.push_back((uint32_t)sc.Objects.size());
                    for (int e = 0; e < 16; e++) ao.BindingGlobals.push_back((float)mn->GlobalTransform.m[e / 4][e % 4]);
                    auto sk = skinOf.find(mn->NodeName);
                    if (sk != skinOf.end()) {
                        AnimatedObject::Skin s; s.MeshNode = rig->FindNode(mn->NodeName); s.SceneNode = ni;
                        for (const std::string& jn : sk->second->Names) s.JointNodes.push_back(rig->FindNode(jn));
                        for (const auto& mtx : sk->second->InverseBindMatrices) s.InverseBinds.insert(s.InverseBinds.end(), mtx.begin(), mtx.end());
                        ao.Skins.push_back(std::move(s));
                    }
                }
                sc.Objects.push_back(o);
            }
            if (rig) sc.Animations.push_back(std::move(ao));
        }
    return sc;
}

} // namespace ptamd::ingest
