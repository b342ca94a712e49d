// Stand-alone fuzz driver for the code that reads untrusted bytes: the bitmap decoders (csrc/image_decode.cpp, jpeg_decode.cpp)
// and the scene readers (csrc/scene_parser.cpp, json_min.h).  An ordinary host program: compiled together with image_decode.cpp,
// jpeg_decode.cpp, scene.cpp and scene_parser.cpp, no HIP, none of the project's shared library, never loaded into Python.
// tests/test_reader_fuzz.py builds it twice -- with the project's host flags, and with -fsanitize=address,undefined -- and runs it.
//
//   fuzz_readers bitmaps|scenes GOLDEN_DIR SEED COUNT [--only BASE --case N]
//
// COUNT mutated inputs per base input; case N of base B under seed S is the same bytes on every machine (own xorshift generator,
// one state per case), so a failure names what replays it.  One summary line: tried, accepted, rejected.  Exit status 1 on the
// first violated rule:
//   * a decode that returns has width > 0, height > 0, channels in 1..4, width x height <= 2^28, pixels.size() == w x h x channels;
//   * a scene that returns has every triangle index below its mesh's vertex count, index counts that are multiples of three,
//     normals and uvs absent or one per vertex, every material's texture reference absent or in range (a mesh's material index
//     outside the materials is, by include/crt_hip.h, "no material" -- the kernels test it -- so such meshes are only counted);
//   * a call that does not return throws std::runtime_error: std::bad_alloc, std::length_error, any other exception is a failure;
//   * (plain build only) the heap a decode holds at its peak stays within crt::decodeHeapBound(file): global operator new is
//     replaced by a counting one that REFUSES the request that would pass the bound, so a decoder that trusts a header fails here
//     at once instead of zero-filling gigabytes.  The sanitized build keeps the sanitizer's allocator.
#include "../directx-raytracer_amd/csrc/image_decode.h"
#include "../directx-raytracer_amd/csrc/scene.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include <dirent.h>
#include <unistd.h>

#if defined(__SANITIZE_ADDRESS__)
#define FUZZ_SANITIZED 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define FUZZ_SANITIZED 1
#endif
#endif

// ------------------------------------------------------------------------------------------------ heap accounting (plain build)
namespace heap {
size_t current = 0, peak = 0;
size_t limit = 0;    // 0: unlimited; else the most `current` may reach
size_t refused = 0;  // the size of the first request refused under `limit`
}

#ifndef FUZZ_SANITIZED
namespace {
constexpr size_t kHead = 16; // keeps malloc's alignment
void* counted(size_t n)
{
    if (heap::limit && (n > heap::limit || heap::current + n > heap::limit)) {
        if (!heap::refused) heap::refused = n;
        throw std::bad_alloc();
    }
    void* raw = std::malloc(n + kHead);
    if (!raw) throw std::bad_alloc();
    std::memcpy(raw, &n, sizeof(n));
    heap::current += n;
    if (heap::current > heap::peak) heap::peak = heap::current;
    return static_cast<char*>(raw) + kHead;
}
void release(void* p) noexcept
{
    if (!p) return;
    void* raw = static_cast<char*>(p) - kHead;
    size_t n;
    std::memcpy(&n, raw, sizeof(n));
    heap::current -= n;
    std::free(raw);
}
} // namespace
void* operator new(size_t n) { return counted(n); }
void* operator new[](size_t n) { return counted(n); }
void operator delete(void* p) noexcept { release(p); }
void operator delete[](void* p) noexcept { release(p); }
void operator delete(void* p, size_t) noexcept { release(p); }
void operator delete[](void* p, size_t) noexcept { release(p); }
#endif

namespace {

using Bytes = std::vector<unsigned char>;

// ------------------------------------------------------------------------------------------------ generator
struct Rng {
    uint64_t s;
    uint64_t next() // xorshift64*
    {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    size_t below(size_t n) { return n ? static_cast<size_t>(next() % n) : 0; }
};

uint64_t fnv(const std::string& t)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned char c : t) h = (h ^ c) * 0x100000001b3ull;
    return h;
}

Rng caseRng(uint64_t seed, const std::string& base, uint64_t n)
{
    Rng r{ (seed * 0x9E3779B97F4A7C15ull) ^ fnv(base) ^ (n * 0xD1B54A32D192ED03ull) };
    if (!r.s) r.s = 1;
    for (int i = 0; i < 4; i++) r.next();
    return r;
}

// ------------------------------------------------------------------------------------------------ general mutators
const char* const kMutatorNames[] = { "truncate", "random-bytes", "boundary-byte", "copy-span", "insert", "aimed" };
const unsigned char kBoundaryBytes[] = { 0, 1, 0x7f, 0x80, 0xfe, 0xff, 8, 16, 32 };

void mutateGeneral(Bytes& b, int which, Rng& r)
{
    if (b.empty()) return;
    switch (which) {
    case 0: b.resize(r.below(b.size())); break;
    case 1:
        for (size_t k = 1 + r.below(4); k; k--) b[r.below(b.size())] = static_cast<unsigned char>(r.next());
        break;
    case 2: b[r.below(b.size() < 64 ? b.size() : 64)] = kBoundaryBytes[r.below(sizeof(kBoundaryBytes))]; break;
    case 3: {
        const size_t len = 1 + r.below(b.size() < 32 ? b.size() : 32), from = r.below(b.size() - len + 1), to = r.below(b.size() - len + 1);
        std::memmove(&b[to], &b[from], len);
        break;
    }
    default: {
        Bytes ins(1 + r.below(8));
        for (unsigned char& c : ins) c = static_cast<unsigned char>(r.next());
        b.insert(b.begin() + static_cast<std::ptrdiff_t>(r.below(b.size() + 1)), ins.begin(), ins.end());
    }
    }
}

// ------------------------------------------------------------------------------------------------ size fields
// boundary values for one size field, and pairs (width, height) whose PRODUCT sits on a boundary: 2^28 (the texel cap), just above
// it, 2^32, 2^62 .. 2^64 (where a 64-bit product wraps), and the pair that wrapped the PNG check.  A binary field takes the values
// that fit its width; decimal fields (PNM, HDR) take them all, and longer digit strings besides.
const uint64_t kSingles[] = { 0, 1, 1ull << 14, (1ull << 15) - 1, (1ull << 16) - 1, (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 1,
                              0xFFFFC000ull /* -2^14 as a BMP height */, 0xFFFFFFF9ull /* -7 */ };
const uint64_t kPairs[][2] = { { 1ull << 14, 1ull << 14 }, { 1ull << 14, (1ull << 14) + 1 }, { 17, 15790321 } /* 2^28 + 1 */, { 1ull << 13, 1ull << 15 },
                               { 1ull << 16, 1ull << 16 }, { (1ull << 16) - 1, (1ull << 16) - 1 }, { 1ull << 31, 1ull << 31 }, { (1ull << 32) - 1, (1ull << 32) - 1 },
                               { 3688618971ull, 3688562688ull }, { 1ull << 31, 1ull << 32 } /* 2^63 */, { 1ull << 32, 1ull << 32 } /* 2^64 */,
                               { 8589934592ull, 2147483648ull } /* 2^64 again, ten digits each */ };
const char* const kLongDigits[] = { "18446744073709551616", "99999999999999999999", "4294967296", "00000000001", "340282366920938463463374607431768211456" };

void put(Bytes& b, size_t at, int bytes, bool big, uint64_t v)
{
    if (at + static_cast<size_t>(bytes) > b.size()) return;
    for (int i = 0; i < bytes; i++) b[at + static_cast<size_t>(big ? bytes - 1 - i : i)] = static_cast<unsigned char>(v >> (8 * i));
}

// a pair of binary fields of `bytes` bytes each at `wAt`, `hAt`
void aimBinary(Bytes& b, size_t wAt, size_t hAt, int bytes, bool big, Rng& r)
{
    const uint64_t top = bytes == 2 ? 0xFFFFull : 0xFFFFFFFFull;
    for (int tries = 0; tries < 64; tries++) {
        if (r.below(2)) {
            const uint64_t v = kSingles[r.below(sizeof(kSingles) / sizeof(kSingles[0]))];
            if (v > top) continue;
            put(b, r.below(2) ? wAt : hAt, bytes, big, v);
        } else {
            const uint64_t* p = kPairs[r.below(sizeof(kPairs) / sizeof(kPairs[0]))];
            if (p[0] > top || p[1] > top) continue;
            const bool swap = r.below(2) != 0;
            put(b, wAt, bytes, big, p[swap ? 1 : 0]);
            put(b, hAt, bytes, big, p[swap ? 0 : 1]);
        }
        return;
    }
}

// decimal fields: the text of a (width, height) pair
void aimDecimal(std::string& w, std::string& h, Rng& r)
{
    const size_t kind = r.below(5);
    if (kind < 2) {
        (r.below(2) ? w : h) = std::to_string(kSingles[r.below(sizeof(kSingles) / sizeof(kSingles[0]))]);
    } else if (kind < 4) {
        const uint64_t* p = kPairs[r.below(sizeof(kPairs) / sizeof(kPairs[0]))];
        const bool swap = r.below(2) != 0;
        w = std::to_string(p[swap ? 1 : 0]);
        h = std::to_string(p[swap ? 0 : 1]);
    } else {
        (r.below(2) ? w : h) = kLongDigits[r.below(sizeof(kLongDigits) / sizeof(kLongDigits[0]))];
    }
}

bool hasSuffix(const std::string& s, const char* suffix)
{
    const size_t n = std::strlen(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

unsigned be16(const Bytes& b, size_t at) { return (static_cast<unsigned>(b[at]) << 8) | b[at + 1]; }

// overwrite the size fields of the format `b` is in; false when the fields are not where a well-formed file has them
bool mutateAimedBitmap(Bytes& b, const std::string& name, Rng& r)
{
    if (hasSuffix(name, ".png")) { // IHDR (this decoder does not verify chunk checksums: nothing to recompute)
        if (b.size() < 33) return false;
        aimBinary(b, 16, 20, 4, true, r);
        return true;
    }
    if (hasSuffix(name, ".bmp")) {
        if (b.size() < 26) return false;
        if (b[14] == 12) aimBinary(b, 18, 20, 2, false, r);
        else aimBinary(b, 18, 22, 4, false, r); // (0x80000000 .. 0xFFFFFFFF are negative heights)
        return true;
    }
    if (hasSuffix(name, ".tga")) {
        aimBinary(b, 12, 14, 2, false, r);
        return true;
    }
    if (hasSuffix(name, ".psd")) {
        aimBinary(b, 18, 14, 4, true, r);
        return true;
    }
    if (hasSuffix(name, ".pic")) {
        aimBinary(b, 92, 94, 2, true, r);
        return true;
    }
    if (hasSuffix(name, ".gif")) {
        if (b.size() < 13) return false;
        if (r.below(2)) {
            aimBinary(b, 6, 8, 2, false, r); // the canvas
            return true;
        }
        size_t at = 13 + ((b[10] & 0x80) ? 3u * (2u << (b[10] & 7)) : 0u);
        while (at + 2 < b.size() && b[at] == 0x21) { // extensions in front of the first image
            at += 2;
            while (at < b.size() && b[at]) at += 1u + b[at];
            at++;
        }
        if (at + 9 >= b.size() || b[at] != 0x2C) return false;
        if (r.below(2)) aimBinary(b, at + 5, at + 7, 2, false, r); // the image's extent
        else aimBinary(b, at + 1, at + 3, 2, false, r);            // ... and its place on the canvas
        return true;
    }
    if (hasSuffix(name, ".jpg")) { // the frame header: FF C0 / C1 / C2, length, precision, height, width
        size_t at = 2;
        while (at + 9 < b.size() && b[at] == 0xFF) {
            const unsigned m = b[at + 1];
            if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
                aimBinary(b, at + 7, at + 5, 2, true, r);
                return true;
            }
            at += 2 + be16(b, at + 2);
        }
        return false;
    }
    if (hasSuffix(name, ".ppm") || hasSuffix(name, ".pgm")) { // "P6 <w> <h> <max><one whitespace byte>data"
        size_t at = 2;
        std::string field[3];
        for (std::string& t : field) {
            while (at < b.size() && (b[at] == ' ' || b[at] == '\n' || b[at] == '\r' || b[at] == '\t')) at++;
            while (at < b.size() && b[at] >= '0' && b[at] <= '9') t.push_back(static_cast<char>(b[at++]));
            if (t.empty()) return false;
        }
        aimDecimal(field[0], field[1], r);
        const std::string head = std::string(1, 'P') + static_cast<char>(b[1]) + (r.below(2) ? "\n" : " ") + field[0] + " " + field[1] + "\n" + field[2];
        Bytes out(head.begin(), head.end());
        out.insert(out.end(), b.begin() + static_cast<std::ptrdiff_t>(at), b.end());
        b.swap(out);
        return true;
    }
    if (hasSuffix(name, ".hdr")) { // the "-Y <h> +X <w>" line
        const std::string text(b.begin(), b.end());
        const size_t at = text.find("\n-Y ");
        const size_t end = at == std::string::npos ? at : text.find('\n', at + 1);
        if (end == std::string::npos) return false;
        const size_t plus = text.find(" +X ", at);
        if (plus == std::string::npos || plus > end) return false;
        std::string h = text.substr(at + 4, plus - at - 4), w = text.substr(plus + 4, end - plus - 4);
        aimDecimal(w, h, r);
        const std::string out = text.substr(0, at + 4) + h + " +X " + w + text.substr(end);
        b.assign(out.begin(), out.end());
        return true;
    }
    return false;
}

// ------------------------------------------------------------------------------------------------ reporting
struct Where {
    const char* mode;
    std::string base;
    uint64_t seed, n;
    const char* mutator;
};

[[noreturn]] void fail(const Where& w, const std::string& what)
{
    std::printf("FAIL %s base=%s case=%llu seed=%llu mutator=%s: %s\n", w.mode, w.base.c_str(), static_cast<unsigned long long>(w.n),
                static_cast<unsigned long long>(w.seed), w.mutator, what.c_str());
    std::printf("replay: fuzz_readers %s GOLDEN_DIR %llu 1 --only %s --case %llu\n", w.mode, static_cast<unsigned long long>(w.seed), w.base.c_str(),
                static_cast<unsigned long long>(w.n));
    std::fflush(stdout);
    std::exit(1);
}

struct Tally { uint64_t tried = 0, accepted = 0, rejected = 0, peakOverAll = 0, maxBound = 0, noMaterial = 0; };

// inside a handler: what was thrown, "" for the one kind a reader may throw
const char* const kBadAlloc = "threw std::bad_alloc";
std::string thrown()
{
    try {
        throw;
    } catch (const std::runtime_error&) {
        return "";
    } catch (const std::bad_alloc&) {
        return kBadAlloc;
    } catch (const std::length_error& e) {
        return std::string("threw std::length_error: ") + e.what();
    } catch (const std::logic_error& e) {
        return std::string("threw std::logic_error: ") + e.what();
    } catch (const std::exception& e) {
        return std::string("threw an exception that is no std::runtime_error: ") + e.what();
    } catch (...) {
        return "threw a foreign exception";
    }
}

// ------------------------------------------------------------------------------------------------ one decode, all rules
void checkDecode(const Bytes& file, const std::string& name, const Where& w, Tally& t)
{
    t.tried++;
    const size_t bound = crt::decodeHeapBound(file, name);
    if (bound > t.maxBound) t.maxBound = bound;
    const size_t before = heap::current;
    heap::peak = before;
    heap::refused = 0;
#ifndef FUZZ_SANITIZED
    heap::limit = before + bound;
#endif
    bool ok = false;
    std::string problem;
    try {
        const crt::DecodedImage img = crt::decodeImage(file, name);
        heap::limit = 0;
        ok = true;
        const long long W = img.width, H = img.height, C = img.channels;
        if (W <= 0 || H <= 0 || C < 1 || C > 4 || W * H > (1ll << 28) || img.pixels.size() != static_cast<size_t>(W * H * C))
            problem = "decoded " + std::to_string(W) + " x " + std::to_string(H) + " x " + std::to_string(C) + " with " + std::to_string(img.pixels.size()) + " bytes of pixels";
    } catch (...) {
        heap::limit = 0;
        problem = thrown();
        if (problem == kBadAlloc && heap::refused)
            problem = "asked for " + std::to_string(heap::refused) + " bytes with " + std::to_string(heap::peak - before) + " held: past the format's heap bound of " +
                      std::to_string(bound) + " for this file of " + std::to_string(file.size()) + " bytes";
    }
    if (!problem.empty()) fail(w, problem);
    if (heap::peak - before > t.peakOverAll) t.peakOverAll = heap::peak - before;
    (ok ? t.accepted : t.rejected)++;
}

// ------------------------------------------------------------------------------------------------ fixed bitmap cases
Bytes str(const std::string& s) { return Bytes(s.begin(), s.end()); }

void be32put(Bytes& b, uint32_t v)
{
    for (int i = 3; i >= 0; i--) b.push_back(static_cast<unsigned char>(v >> (8 * i)));
}

void chunk(Bytes& png, const char* type, const Bytes& data)
{
    be32put(png, static_cast<uint32_t>(data.size()));
    png.insert(png.end(), type, type + 4);
    png.insert(png.end(), data.begin(), data.end());
    be32put(png, 0); // (the checksum is not read)
}

Bytes pngWith(uint32_t w, uint32_t h, unsigned depth, unsigned color, const Bytes* trns, const Bytes* idat)
{
    static const unsigned char magic[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
    Bytes png(magic, magic + 8), ihdr;
    be32put(ihdr, w);
    be32put(ihdr, h);
    ihdr.push_back(static_cast<unsigned char>(depth));
    ihdr.push_back(static_cast<unsigned char>(color));
    ihdr.insert(ihdr.end(), 3, 0);
    chunk(png, "IHDR", ihdr);
    if (trns) chunk(png, "tRNS", *trns);
    if (idat) chunk(png, "IDAT", *idat);
    chunk(png, "IEND", Bytes());
    return png;
}

// a zlib stream of one stored block
Bytes stored(const Bytes& raw)
{
    Bytes z = { 0x78, 0x01, 0x01, static_cast<unsigned char>(raw.size()), static_cast<unsigned char>(raw.size() >> 8),
                static_cast<unsigned char>(~raw.size()), static_cast<unsigned char>(~raw.size() >> 8) };
    z.insert(z.end(), raw.begin(), raw.end());
    z.insert(z.end(), 4, 0); // (the Adler sum is not read)
    return z;
}

struct Fixed { std::string name; Bytes file; };

std::vector<Fixed> fixedBitmaps()
{
    std::vector<Fixed> out;
    Bytes tga(18, 0);
    tga[2] = 2; tga[12] = tga[13] = tga[14] = tga[15] = 0xFF; tga[16] = 32;
    out.push_back({ "fixed_65535x65535_32bit_header_only.tga", tga });
    tga[12] = 0; tga[13] = 0x10; tga[14] = 0; tga[15] = 0x10; tga[16] = 24;
    out.push_back({ "fixed_4096x4096_raw_no_data.tga", tga });
    out.push_back({ "fixed_2pow33_x_2pow31.pgm", str("P5 8589934592 2147483648 255\n") });
    out.push_back({ "fixed_65536x65536.ppm", str("P6 65536 65536 255\n") });
    const Bytes emptyStream = { 0x78, 0x9C, 0x03, 0x00, 0x00, 0x00, 0x00, 0x01 }, none;
    out.push_back({ "fixed_3688618971x3688562688.png", pngWith(3688618971u, 3688562688u, 8, 2, nullptr, &emptyStream) });
    out.push_back({ "fixed_16384x16384_rgba16_idat_of_no_bytes.png", pngWith(16384, 16384, 16, 6, nullptr, &none) });
    out.push_back({ "fixed_16384x16384_rgba16_idat_of_an_empty_stream.png", pngWith(16384, 16384, 16, 6, nullptr, &emptyStream) });
    return out;
}

// 16-bit colour keys are compared on the full samples: three texels -- the key itself, the key's high bytes with other low bytes,
// other high bytes -- must come back transparent, opaque, opaque
void checkColourKey16(Tally& t)
{
    const Bytes greyKey = { 0x75, 0x30 }, greyRow = { 0, 0x75, 0x30, 0x75, 0x31, 0x76, 0x30 };
    const Bytes rgbKey = { 0x12, 0x34, 0x56, 0x78, 0x9A, 0xBC };
    const Bytes rgbRow = { 0, 0x12, 0x34, 0x56, 0x78, 0x9A, 0xBC, 0x12, 0x34, 0x56, 0x78, 0x9A, 0xBD, 0x12, 0x34, 0x57, 0x78, 0x9A, 0xBC };
    const struct { const char* name; unsigned color; const Bytes* key; const Bytes* row; int channels; } cases[2] = {
        { "fixed_grey16_key.png", 0, &greyKey, &greyRow, 2 }, { "fixed_rgb16_key.png", 2, &rgbKey, &rgbRow, 4 } };
    for (const auto& c : cases) {
        const Bytes z = stored(*c.row);
        const Bytes png = pngWith(3, 1, 16, c.color, c.key, &z);
        const Where w{ "bitmaps", c.name, 0, 0, "fixed" };
        t.tried++;
        crt::DecodedImage img;
        try {
            img = crt::decodeImage(png, c.name);
        } catch (const std::exception& e) {
            fail(w, std::string("a well-formed file was refused: ") + e.what());
        }
        t.accepted++;
        if (img.width != 3 || img.height != 1 || img.channels != c.channels || img.pixels.size() != static_cast<size_t>(3 * c.channels)) fail(w, "wrong extent");
        const unsigned a0 = img.pixels[static_cast<size_t>(c.channels - 1)], a1 = img.pixels[static_cast<size_t>(2 * c.channels - 1)], a2 = img.pixels[static_cast<size_t>(3 * c.channels - 1)];
        if (a0 != 0 || a1 != 255 || a2 != 255)
            fail(w, "alpha " + std::to_string(a0) + ", " + std::to_string(a1) + ", " + std::to_string(a2) + " for the key, the key's high bytes alone, another colour: expected 0, 255, 255");
    }
}

Bytes slurp(const std::string& path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) {
        std::printf("cannot read %s\n", path.c_str());
        std::exit(2);
    }
    return Bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

int runBitmaps(const std::string& golden, uint64_t seed, uint64_t count, const std::string& only, long long onlyCase)
{
    std::vector<std::string> names;
    if (DIR* d = opendir(golden.c_str())) {
        while (const dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.compare(0, 3, "tex") == 0 && n != "tex_rgb8_big.png" && !hasSuffix(n, ".json")) names.push_back(n);
        }
        closedir(d);
    }
    if (names.empty()) {
        std::printf("no tex* fixtures under %s\n", golden.c_str());
        return 2;
    }
    // sorted: the order of a directory listing differs between machines
    for (size_t i = 0; i < names.size(); i++)
        for (size_t j = i + 1; j < names.size(); j++)
            if (names[j] < names[i]) names[i].swap(names[j]);
    Tally t;
    for (const Fixed& f : fixedBitmaps()) { // (--only NAME runs one of them alone)
        if (!only.empty() && only != f.name) continue;
        const Where w{ "bitmaps", f.name, 0, 0, "fixed" };
        const uint64_t acceptedBefore = t.accepted;
        checkDecode(f.file, f.name, w, t);
        if (t.accepted != acceptedBefore) fail(w, "a file that must be refused was decoded");
    }
    if (only.empty() || only == "fixed_colour_key16") checkColourKey16(t);
    uint64_t aimed = 0, aimedAccepted = 0;
    for (const std::string& name : names) {
        if (!only.empty() && name != only) continue;
        const Bytes base = slurp(golden + "/" + name);
        for (uint64_t n = 0; n < count; n++) {
            if (onlyCase >= 0 && n != static_cast<uint64_t>(onlyCase)) continue;
            Rng r = caseRng(seed, name, n);
            Bytes b = base;
            int which = static_cast<int>(r.below(6));
            if (which == 5 && !mutateAimedBitmap(b, name, r)) which = 1;
            if (which < 5) mutateGeneral(b, which, r);
            const Where w{ "bitmaps", name, seed, n, kMutatorNames[which] };
            const uint64_t acceptedBefore = t.accepted;
            checkDecode(b, name, w, t);
            if (which == 5) {
                aimed++;
                aimedAccepted += t.accepted - acceptedBefore;
            }
        }
    }
    std::printf("bitmaps: bases=%zu tried=%llu accepted=%llu rejected=%llu aimed=%llu aimed_accepted=%llu peak_heap=%llu largest_bound=%llu\n", names.size(),
                static_cast<unsigned long long>(t.tried), static_cast<unsigned long long>(t.accepted), static_cast<unsigned long long>(t.rejected),
                static_cast<unsigned long long>(aimed), static_cast<unsigned long long>(aimedAccepted), static_cast<unsigned long long>(t.peakOverAll), static_cast<unsigned long long>(t.maxBound));
    return 0;
}

// ------------------------------------------------------------------------------------------------ scenes
// every key the .crtscene reader reads: settings, camera, lights, texture-named and literal albedos, the texture kinds that need
// no file, two objects of which one has uvs
const char* const kSceneJson =
    "{\"settings\":{\"background_color\":[0.1,0.2,0.3],\"image_settings\":{\"width\":64,\"height\":48}},\n"
    "\"camera\":{\"matrix\":[1,0,0,0,1,0,0,0,1],\"position\":[0,1.5,4]},\n"
    "\"lights\":[{\"intensity\":170,\"position\":[2,3,4]},{\"intensity\":25.5,\"position\":[-2,3,1]}],\n"
    "\"materials\":[{\"type\":\"diffuse\",\"albedo\":\"chk\",\"smooth_shading\":false},{\"type\":\"reflective\",\"albedo\":[0.9,0.8,0.7],\"smooth_shading\":true},"
    "{\"type\":\"refractive\",\"ior\":1.5,\"smooth_shading\":false},{\"type\":\"constant\",\"albedo\":\"edg\"},{\"type\":\"diffuse\",\"albedo\":\"missing\"}],\n"
    "\"textures\":[{\"name\":\"alb\",\"type\":\"albedo\",\"albedo\":[0.1,0.2,0.3]},"
    "{\"name\":\"edg\",\"type\":\"edges\",\"edge_color\":[1,1,1],\"inner_color\":[0,0,0],\"edge_width\":0.05},"
    "{\"name\":\"chk\",\"type\":\"checker\",\"color_A\":[1,0,0],\"color_B\":[0,1,0],\"square_size\":0.25}],\n"
    "\"objects\":[{\"material_index\":0,\"vertices\":[0,0,0, 1,0,0, 0,1,0, 1,1,0],\"triangles\":[0,1,2, 1,3,2],\"uvs\":[0,0,0, 1,0,0, 0,1,0, 1,1,0]},"
    "{\"material_index\":3,\"vertices\":[-1,-1,-1, 1,-1,-1, 1,1,-1, -1,1,-1, 0,0,1],\"triangles\":[0,1,4, 1,2,4, 2,3,4, 3,0,4, 0,2,1, 0,3,2]}]}\n";

// v, vn, vt, negative indices, a quad, the a/b/c and a//c forms, two groups
const char* const kSceneObj =
    "# fuzz base\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n"
    "f 1/1/1 2/2/1 3/3/1 4/4/1\nf 1//1 3//1 4//1\no second\nv 0 0 1\nv 1 0 1\nv 0 1 1\nvn 0 1 0\nf -3/1/2 -2/2/2 -1/3/2\nf -3 -1 -2\ng third\nf 5 6 7\n";

const char* const kNumberTokens[] = { "-1", "0", "1", "3", "4", "5", "2147483647", "2147483648", "4294967296", "-2147483649", "1e9", "1e308", "1e-320",
                                      "-0", "0.5", "99999999999999999999", "1e99999" };

// swap one number of a text for a boundary number: reaches the index and count checks that byte noise rarely gets to
bool mutateNumberToken(Bytes& b, Rng& r)
{
    std::vector<std::pair<size_t, size_t>> spans;
    for (size_t i = 0; i < b.size();) {
        if ((b[i] >= '0' && b[i] <= '9') || (b[i] == '-' && i + 1 < b.size() && b[i + 1] >= '0' && b[i + 1] <= '9')) {
            size_t j = i + 1;
            while (j < b.size() && ((b[j] >= '0' && b[j] <= '9') || b[j] == '.')) j++;
            spans.emplace_back(i, j);
            i = j;
        } else {
            i++;
        }
    }
    if (spans.empty()) return false;
    const auto span = spans[r.below(spans.size())];
    const std::string tok = kNumberTokens[r.below(sizeof(kNumberTokens) / sizeof(kNumberTokens[0]))];
    b.erase(b.begin() + static_cast<std::ptrdiff_t>(span.first), b.begin() + static_cast<std::ptrdiff_t>(span.second));
    b.insert(b.begin() + static_cast<std::ptrdiff_t>(span.first), tok.begin(), tok.end());
    return true;
}

// the counts, string lengths and offsets of a well-formed .crtbin (the layout SceneParser::saveBinary writes), and its triangle indices
struct BinField { size_t at; int bytes; };

bool walkBinary(const Bytes& b, std::vector<BinField>& counts, std::vector<size_t>& indices)
{
    size_t at = 8 + 12 + 8 + 12 + 36;
    auto u32 = [&](bool record) -> uint64_t {
        if (at + 4 > b.size()) return ~0ull;
        uint32_t v;
        std::memcpy(&v, &b[at], 4);
        if (record) counts.push_back({ at, 4 });
        at += 4;
        return v;
    };
    auto u64 = [&]() -> uint64_t {
        if (at + 8 > b.size()) return ~0ull;
        uint64_t v;
        std::memcpy(&v, &b[at], 8);
        counts.push_back({ at, 8 });
        at += 8;
        return v;
    };
    auto skipStr = [&]() { const uint64_t n = u32(true); if (n != ~0ull) at += n; };
    uint64_t n = u32(true); // lights
    if (n == ~0ull) return false;
    at += 16 * n;
    n = u32(true); // materials
    if (n == ~0ull) return false;
    for (uint64_t i = 0; i < n; i++) { at += 4 + 12 + 4 + 4; skipStr(); }
    n = u32(true); // textures
    if (n == ~0ull) return false;
    for (uint64_t i = 0; i < n; i++) { skipStr(); skipStr(); at += 12 + 12 + 4; skipStr(); }
    n = u32(true); // meshes
    if (n == ~0ull) return false;
    for (uint64_t i = 0; i < n; i++) {
        at += 4;
        const uint64_t nv = u64(), ni = u64(), nn = u64(), nu = u64();
        if (nu == ~0ull) return false;
        at += 12 * nv;
        for (uint64_t k = 0; k < ni; k++) indices.push_back(at + 4 * k);
        at += 4 * ni + 12 * nn + 12 * nu;
    }
    return at == b.size();
}

const uint64_t kCountValues[] = { 0, 1, 2, 3, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull, 0x100000000ull, 0x1555555555555556ull /* 2^64 / 12 + 1 */,
                                  0x4000000000000000ull /* 2^64 / 4 */, 0x7FFFFFFFFFFFFFFFull, 0x8000000000000000ull, 0xFFFFFFFFFFFFFFFFull };

void mutateAimedBinary(Bytes& b, const std::vector<BinField>& counts, const std::vector<size_t>& indices, Rng& r)
{
    if (r.below(3) == 0 && !indices.empty()) { // a triangle index: the vertex count, one below zero, the largest int
        static const uint32_t values[] = { 3, 4, 5, 0xFFFFFFFFu, 0x7FFFFFFFu, 0x80000000u };
        const uint32_t v = values[r.below(6)];
        std::memcpy(&b[indices[r.below(indices.size())]], &v, 4);
        return;
    }
    const BinField f = counts[r.below(counts.size())];
    uint64_t v = kCountValues[r.below(sizeof(kCountValues) / sizeof(kCountValues[0]))];
    if (r.below(3) == 0) { // one more or one less than what the file holds
        uint64_t old = 0;
        std::memcpy(&old, &b[f.at], static_cast<size_t>(f.bytes));
        v = r.below(2) ? old + 1 : old - 1;
    }
    std::memcpy(&b[f.at], &v, static_cast<size_t>(f.bytes));
}

void checkScene(int format, const Bytes& input, const Where& w, Tally& t)
{
    t.tried++;
    const std::string text(input.begin(), input.end());
    std::string problem;
    bool ok = false;
    try {
        crt::Scene scene;
        if (format == 0) crt::SceneParser::parseCrtscene(text, scene);
        else if (format == 1) crt::SceneParser::parseObj(text, scene);
        else crt::SceneParser::parseBinary(text, scene);
        ok = true;
        const size_t nMaterials = scene.getMaterials().size(), nTextures = scene.getTextures().size();
        size_t m = 0;
        for (const crt::Mesh& mesh : scene.getObjects()) {
            const size_t nv = mesh.getVertices().size();
            const std::string at = "mesh " + std::to_string(m++) + ": ";
            if (mesh.getIndices().size() % 3 != 0) problem = at + "index count that is no multiple of three";
            for (int k : mesh.getIndices())
                if (k < 0 || static_cast<size_t>(k) >= nv) problem = at + "triangle index " + std::to_string(k) + " with " + std::to_string(nv) + " vertices";
            if (!mesh.getVertexNormals().empty() && mesh.getVertexNormals().size() != nv) problem = at + std::to_string(mesh.getVertexNormals().size()) + " normals for " + std::to_string(nv) + " vertices";
            if (!mesh.getUV().empty() && mesh.getUV().size() != nv) problem = at + std::to_string(mesh.getUV().size()) + " uvs for " + std::to_string(nv) + " vertices";
            const int mi = mesh.getMaterialIndex();
            if (mi < 0 || static_cast<size_t>(mi) >= nMaterials) t.noMaterial++; // "no material" by the C ABI's contract
        }
        for (const crt::Material& mat : scene.getMaterials()) {
            const int ti = mat.isTexture() ? scene.textureIndexByName(mat.getTextureName()) : -1; // as crt_scene_material resolves it
            if (ti != -1 && (ti < 0 || static_cast<size_t>(ti) >= nTextures)) problem = "material with texture index " + std::to_string(ti) + " of " + std::to_string(nTextures);
            if (static_cast<unsigned>(mat.getType()) > 4u) problem = "material of type " + std::to_string(static_cast<unsigned>(mat.getType()));
        }
    } catch (...) {
        problem = thrown();
    }
    if (!problem.empty()) fail(w, problem);
    (ok ? t.accepted : t.rejected)++;
}

int runScenes(uint64_t seed, uint64_t count, const std::string& only, long long onlyCase)
{
    // the third base: what saveBinary writes for the parsed document
    char path[] = "/tmp/fuzz_readers_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) {
        std::printf("cannot create a temporary file\n");
        return 2;
    }
    close(fd);
    Bytes bin;
    {
        crt::Scene scene;
        crt::SceneParser::parseCrtscene(kSceneJson, scene);
        crt::SceneParser::saveBinary(path, scene);
        bin = slurp(path);
        unlink(path);
    }
    std::vector<BinField> counts;
    std::vector<size_t> indices;
    if (!walkBinary(bin, counts, indices) || counts.size() < 20 || indices.size() != 24) {
        std::printf("the .crtbin base does not have the layout this driver walks\n");
        return 2;
    }
    const struct { const char* name; Bytes bytes; } bases[3] = { { "base.crtscene", str(kSceneJson) }, { "base.obj", str(kSceneObj) }, { "base.crtbin", bin } };
    Tally t;
    uint64_t acceptedPer[3] = { 0, 0, 0 };
    for (int format = 0; format < 3; format++) {
        if (!only.empty() && only != bases[format].name) continue;
        const Where whole{ "scenes", bases[format].name, seed, 0, "none" };
        const uint64_t acceptedBefore = t.accepted;
        checkScene(format, bases[format].bytes, whole, t);
        if (t.accepted == acceptedBefore) fail(whole, "the unmutated base was refused");
        for (uint64_t n = 0; n < count; n++) {
            if (onlyCase >= 0 && n != static_cast<uint64_t>(onlyCase)) continue;
            Rng r = caseRng(seed, bases[format].name, n);
            Bytes b = bases[format].bytes;
            int which = static_cast<int>(r.below(6));
            if (which == 5) {
                if (format == 2) mutateAimedBinary(b, counts, indices, r);
                else if (!mutateNumberToken(b, r)) which = 1;
            }
            if (which < 5) mutateGeneral(b, which, r);
            const Where w{ "scenes", bases[format].name, seed, n, kMutatorNames[which] };
            const uint64_t before = t.accepted;
            checkScene(format, b, w, t);
            acceptedPer[format] += t.accepted - before;
        }
    }
    std::printf("scenes: bases=3 tried=%llu accepted=%llu rejected=%llu accepted_crtscene=%llu accepted_obj=%llu accepted_crtbin=%llu no_material_meshes=%llu\n",
                static_cast<unsigned long long>(t.tried), static_cast<unsigned long long>(t.accepted), static_cast<unsigned long long>(t.rejected),
                static_cast<unsigned long long>(acceptedPer[0]), static_cast<unsigned long long>(acceptedPer[1]), static_cast<unsigned long long>(acceptedPer[2]),
                static_cast<unsigned long long>(t.noMaterial));
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 5) {
        std::printf("usage: fuzz_readers bitmaps|scenes GOLDEN_DIR SEED COUNT [--only BASE --case N]\n");
        return 2;
    }
    const std::string mode = argv[1], golden = argv[2];
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10), count = std::strtoull(argv[4], nullptr, 10);
    std::string only;
    long long onlyCase = -1;
    for (int i = 5; i + 1 < argc; i += 2) {
        if (std::strcmp(argv[i], "--only") == 0) only = argv[i + 1];
        else if (std::strcmp(argv[i], "--case") == 0) onlyCase = std::strtoll(argv[i + 1], nullptr, 10);
    }
    if (mode == "bitmaps") return runBitmaps(golden, seed, onlyCase >= 0 ? static_cast<uint64_t>(onlyCase) + 1 : count, only, onlyCase);
    if (mode == "scenes") return runScenes(seed, onlyCase >= 0 ? static_cast<uint64_t>(onlyCase) + 1 : count, only, onlyCase);
    std::printf("unknown mode %s\n", mode.c_str());
    return 2;
}
