// CPU sanitizer harness for the Exif-orientation path of csrc/jpeg.hip: msocr_jpeg_parse_oriented_host ->
// msocr_jpeg_entropy_decode_host -> msocr_jpeg_reconstruct_oriented_host.  Built by tests/test_jpeg_orient_cpu.py with
// -fsanitize=address,undefined on the host side only (no GPU).  Seeds: one JPEG per orientation 1..8 (argv order).  Every seed and
// every mutation of its Exif APP1 segment (flipped bytes, rewritten segment length, IFD offset / entry count / entry fields past
// the end, a doubled segment, truncation inside it) is parsed; what parses is decoded into exactly sized heap blocks, the pixels
// into exactly 3 * W * H bytes: an index error of the destination remap is an ASan report, not a silent write.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "msocr.h"

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 11);
}

// 0 = refused somewhere, 1..8 = reconstructed with that orientation, -1 = a contract violation
static int run_one(const std::vector<uint8_t>& d) {
  msocr_jpeg_info info;
  int32_t orientation = -7;
  uint8_t* buf = (uint8_t*)malloc(d.size() ? d.size() : 1);   // exactly sized: a read past the end is an ASan error
  memcpy(buf, d.data(), d.size());
  int result = 0;
  const int rc = msocr_jpeg_parse_oriented_host(buf, (int64_t)d.size(), &info, &orientation);
  if (orientation < 1 || orientation > 8) { fprintf(stderr, "orientation %d out of 1..8 (rc %d)\n", orientation, rc); result = -1; }
  else if (rc == 0 && info.supported && info.coef_total > 0 && info.coef_total < (int64_t)1 << 24 && (int64_t)info.width * info.height < (1 << 22)) {
    int16_t* coef = (int16_t*)malloc((size_t)info.coef_total * 2);
    if (msocr_jpeg_entropy_decode_host(buf, (int64_t)d.size(), &info, coef) == 0) {
      const size_t n = (size_t)3 * info.width * info.height;
      uint8_t* rgb = (uint8_t*)malloc(n);
      memset(rgb, 0xA5, n);
      if (msocr_jpeg_reconstruct_oriented_host(&info, orientation, coef, rgb) != 0) { fprintf(stderr, "reconstruction refused a decoded stream\n"); result = -1; }
      else result = orientation;
      // anything outside 1..8 is an argument error and writes nothing
      if (msocr_jpeg_reconstruct_oriented_host(&info, 0, coef, rgb) == 0 || msocr_jpeg_reconstruct_oriented_host(&info, 9, coef, rgb) == 0) result = -1;
      free(rgb);
    }
    free(coef);
  }
  free(buf);
  return result;
}

int main(int argc, char** argv) {
  long tried = 0, reconstructed = 0, doubled_refused = 0;
  const int rounds = argc > 1 ? atoi(argv[1]) : 200;
  char seen[9] = {0};
  for (int a = 2; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) return 2;
    std::vector<uint8_t> seed;
    uint8_t tmp[4096];
    size_t n;
    while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) seed.insert(seed.end(), tmp, tmp + n);
    fclose(f);
    const int so = run_one(seed);
    if (so < 1) { fprintf(stderr, "seed %s not reconstructed\n", argv[a]); return 3; }
    if (a - 2 < 8) seen[a - 2] = (char)('0' + so);
    ++tried; ++reconstructed;
    // the Exif APP1 segment: FF E1 len len 'E' 'x' 'i' 'f' 0 0 <TIFF header 8 bytes> <IFD>
    size_t seg = 0;
    for (size_t i = 2; i + 10 < seed.size(); ++i)
      if (seed[i] == 0xFF && seed[i + 1] == 0xE1 && memcmp(&seed[i + 4], "Exif\0\0", 6) == 0) { seg = i; break; }
    if (!seg) { fprintf(stderr, "seed %s has no Exif segment\n", argv[a]); return 3; }
    const size_t seg_len = 2 + (((size_t)seed[seg + 2] << 8) | seed[seg + 3]);   // marker + length field + payload
    const size_t tiff = seg + 10;
    for (int r = 0; r < rounds; ++r) {
      std::vector<uint8_t> m = seed;
      const uint32_t kind = rnd() % 7;
      bool doubled = false;
      if (kind == 0) {         // byte flips anywhere in the segment
        const int flips = 1 + rnd() % 4;
        for (int k = 0; k < flips; ++k) m[seg + 4 + rnd() % (seg_len - 4)] = (uint8_t)rnd();
      } else if (kind == 1) {  // the segment's length field
        m[seg + 2] = (uint8_t)rnd(); m[seg + 3] = (uint8_t)rnd();
      } else if (kind == 2) {  // IFD0 offset: past the end, near the end, huge
        const uint32_t v = rnd() % 3 == 0 ? 0xFFFFFFFFu - rnd() % 16 : (rnd() % 2 ? (uint32_t)seg_len - 12 + rnd() % 8 : rnd());
        for (int k = 0; k < 4; ++k) m[tiff + 4 + k] = (uint8_t)(v >> (8 * (rnd() % 2 ? k : 3 - k)));
      } else if (kind == 3) {  // entry count of IFD0 (the seeds' IFD sits at offset 8)
        m[tiff + 8] = (uint8_t)rnd(); m[tiff + 9] = (uint8_t)rnd();
      } else if (kind == 4) {  // fields of the first entries: tag, type, count, value
        const int flips = 1 + rnd() % 6;
        for (int k = 0; k < flips; ++k) { const size_t p = tiff + 10 + rnd() % 24; if (p < seg + seg_len) m[p] = (uint8_t)(rnd() % 4 ? rnd() % 10 : rnd()); }
      } else if (kind == 5) {  // a second Exif segment: the oriented entry must refuse the stream
        m.insert(m.begin() + (long)(seg + seg_len), seed.begin() + (long)seg, seed.begin() + (long)(seg + seg_len));
        doubled = true;
      } else {                 // truncation inside or right behind the segment
        m.resize(seg + rnd() % (seg_len + 8));
      }
      const int o = run_one(m);
      if (o < 0) return 3;
      if (doubled) { if (o != 0) { fprintf(stderr, "a stream with two Exif segments was taken\n"); return 3; } ++doubled_refused; }
      if (o > 0) ++reconstructed;
      ++tried;
    }
  }
  printf("jpeg_orient_fuzz: %ld streams, %ld reconstructed, %ld doubled segments refused; orientations of the seeds: %s\n", tried, reconstructed,
         doubled_refused, seen);
  return 0;
}
