// Bitmap texture files.  The reference loads whatever its vendored stb_image decodes (R/CRTTextureBitmap.cpp:10,
// stbi_load(path, &w, &h, &channels, 0)); stb_image is third party and is not used here.  These decoders cover every format it
// reads -- PNG (all colour types and bit depths, Adam7 interlace, tRNS), JPEG (baseline and progressive, jpeg_decode.cpp), GIF
// (first image), Photoshop PSD (merged RGB image), Radiance HDR (through that decoder's tone curve), Softimage PIC, BMP (palettes,
// 16 / 24 / 32 bit with channel masks, uncompressed), TGA (true colour, grey, colour-mapped; raw and run-length coded), binary
// PPM / PGM -- and yield what stbi_load yields for them, that decoder's oddities included where a texel depends on them: rows top
// to bottom, `channels` bytes per texel in the file's own channel count (1 grey, 2 grey + alpha, 3 RGB, 4 RGBA; 16-bit PNG / PSD
// samples reduced to their high byte, after a 16-bit colour key has been compared with the full samples).  Known answers:
// tests/golden/bitmap_known_answers.json and bitmap_known_answers_more.json, produced by the reference's own CRTTextureBitmap over
// the same 75 files (oracle/make_golden.py).
#pragma once

#include <string>
#include <vector>

namespace crt {

struct DecodedImage {
    int width = 0, height = 0, channels = 0;
    std::vector<unsigned char> pixels; // height x width x channels
};

// `what` names the file in error messages.  Throws std::runtime_error, and nothing else, on anything that is not a well-formed file
// of a supported kind; never reads outside `file`.  Every format holds width x height to 2^28 texels (each factor first, so no
// product wraps), and no decoder allocates on a header's word alone: before the image or an intermediate buffer is allocated the
// file is shown to be long enough to hold that much -- uncoded data byte for byte, coded data by the coding's own ceiling.  The
// heap a decode may hold at its peak, beside `file` itself, is therefore at most kDecodeFixedBytes plus the file's size times
//   PNM      1   every sample is in the file
//   BMP     24   eight one-bit texels a byte, three bytes each
//   TGA    258   raw: every texel is in the file; run-length coded: a packet of two bytes yields 128 texels of up to four bytes;
//                the palette, up to twice its bytes in the file
//   HDR    241   flat: four bytes a texel in the file, fifteen here; coded: a scanline of w texels takes 4 + 8 ceil(w / 127) bytes
//   PSD    256   raw: every sample of the planes that are read; PackBits: two bytes yield 128 samples; four bytes a texel here
//   PIC 153000   a mixed packet's run of 65535 texels takes three bytes and a value; seven bytes a texel here
//   PNG  42400   deflate expands 1032 times at the most (258 bytes for two one-bit codes): the scanline bytes must be within that of
//                the IDAT bytes; a scanline byte holds up to eight texels, a texel takes up to one byte as a sample and four as a result
//   JPEG 26700   every 8 x 8 block of every component takes at least one bit of the file (its DC code, in a sequential file and
//                in a progressive one alike); a block takes 192 bytes of coefficients and samples, up to 16 times that on an image
//                smaller than one MCU, and 64 texels of up to four bytes
//   GIF 327680   the canvas is held to 65536 texels for every byte of the file, the most LZW could draw (a code of one bit stands for
//                at most the 8192 texels of the longest table entry); five bytes a texel here.  No coding bounds a GIF's canvas --
//                the first image may be smaller, and the rest is in no byte of the file -- so this limit is this decoder's own: it
//                refuses a well-formed file whose few bytes name a canvas thousands of times their image, which no texture is.
// (decodeHeapBound below evaluates this for a file).
DecodedImage decodeImage(const std::vector<unsigned char>& file, const std::string& what);

// what no format's bound counts: palettes, code tables, line buffers and error messages
constexpr size_t kDecodeFixedBytes = 512u << 10;
// the bound stated above, evaluated for this file: what decodeImage(file, what) may hold on the heap at its peak (tests/fuzz_readers.cpp
// holds every decode to it)
size_t decodeHeapBound(const std::vector<unsigned char>& file, const std::string& what);

// jpeg_decode.cpp: baseline / progressive Huffman JPEG with the reference decoder's numerical conventions (see the file's header)
DecodedImage decodeJpeg(const std::vector<unsigned char>& file, const std::string& what);

// RFC 1950 / 1951 (zlib stream around deflate), exposed for tests; throws std::runtime_error
std::vector<unsigned char> zlibInflate(const unsigned char* data, size_t size, size_t expectedSize, const std::string& what);

} // namespace crt
