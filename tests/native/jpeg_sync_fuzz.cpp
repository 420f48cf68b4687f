// CPU sanitizer harness for the self-synchronising Huffman stage of csrc/jpeg.hip through its host twin
// (msocr_jpeg_sync_prepare_host + msocr_jpeg_entropy_decode_sync_host: the __host__ __device__ functions the kernels run).
// Built by tests/test_jpeg_sync_cpu.py with -fsanitize=address,undefined on the host pass (no GPU): reads seed JPEGs, damages
// their entropy-coded data (byte writes, truncations, inserted markers) and runs the twin on each with several subsequence lengths
// and round caps, from exactly-sized heap blocks.  The twin's verdict is checked against the serial decoder's on the way:
// refused => status != 0; accepted => same coefficients, or declined (status 2).  Any out-of-bounds access or UB aborts.
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

static long twin_runs = 0, declined = 0, flagged = 0;

static int run_one(const std::vector<uint8_t>& d, int subseq_bytes, int max_rounds) {
  msocr_jpeg_info info;
  uint8_t* buf = (uint8_t*)malloc(d.size() ? d.size() : 1);   // exactly sized: a read past the end is an ASan error
  memcpy(buf, d.data(), d.size());
  int rc = 0;
  if (msocr_jpeg_parse_host(buf, (int64_t)d.size(), &info) == 0 && info.supported && info.coef_total > 0 &&
      info.coef_total < (int64_t)1 << 24) {
    std::vector<int16_t> coef((size_t)info.coef_total);
    const int serial_rc = msocr_jpeg_entropy_decode_host(buf, (int64_t)d.size(), &info, coef.data());
    std::vector<uint64_t> desc((size_t)(msocr_jpeg_scan_desc_bytes() + 7) / 8);
    const int64_t cap = info.coef_total / 64 + 1;
    std::vector<uint32_t> bounds((size_t)(2 * cap));
    const int64_t niv = msocr_jpeg_sync_prepare_host(buf, (int64_t)d.size(), &info, 0, desc.data(), bounds.data(), cap);
    if (niv > 0) {
      std::vector<uint32_t> sub_first((size_t)niv);
      int64_t nsub = 0;
      for (int64_t k = 0; k < niv; ++k) {
        sub_first[(size_t)k] = (uint32_t)nsub;
        const int64_t len = (int64_t)bounds[2 * k + 1] - (int64_t)bounds[2 * k];
        const int64_t n = (len + subseq_bytes - 1) / subseq_bytes;
        nsub += n > 1 ? n : 1;
      }
      int16_t* coef2 = (int16_t*)malloc((size_t)info.coef_total * 2);   // exactly sized too
      int32_t status = -1, rounds = -1;
      const int64_t page_base[4] = {0, 0, 0, nsub};
      if (msocr_jpeg_entropy_decode_sync_host(buf, desc.data(), 1, bounds.data(), sub_first.data(), page_base, subseq_bytes, max_rounds,
                                              coef2, info.coef_total, &status, &rounds) != 0) {
        fprintf(stderr, "the twin refused its arguments\n");
        rc = 1;
      } else if (serial_rc != 0 && status == 0) {
        fprintf(stderr, "the twin took a stream the serial decoder refuses\n");
        rc = 1;
      } else if (serial_rc == 0 && status == 1) {
        fprintf(stderr, "the twin flagged a stream the serial decoder takes\n");
        rc = 1;
      } else if (serial_rc == 0 && status == 0 && memcmp(coef.data(), coef2, coef.size() * 2) != 0) {
        fprintf(stderr, "coefficients differ\n");
        rc = 1;
      }
      declined += status == 2;
      flagged += status == 1;
      ++twin_runs;
      free(coef2);
    } else if (serial_rc == 0) {
      fprintf(stderr, "the prepare step refused a stream the serial decoder takes\n");
      rc = 1;
    }
  }
  free(buf);
  return rc;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 200;
  static const int kSubseq[4] = {16, 48, 256, 1024};
  static const int kCaps[4] = {2, 5, 16, 4096};
  for (int a = 2; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) return 2;
    std::vector<uint8_t> seed;
    uint8_t tmp[4096];
    size_t n;
    while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) seed.insert(seed.end(), tmp, tmp + n);
    fclose(f);
    for (int s = 0; s < 4; ++s)
      if (run_one(seed, kSubseq[s], kCaps[3])) return 3;
    size_t sos = 0;
    for (size_t i = 2; i + 4 < seed.size(); ++i)
      if (seed[i] == 0xFF && seed[i + 1] == 0xDA) { sos = i; break; }
    if (!sos) return 2;
    const size_t body = sos + 14;
    for (int r = 0; r < rounds; ++r) {
      std::vector<uint8_t> m = seed;
      const uint32_t kind = rnd() % 4;
      if (kind == 0) {          // byte writes in the entropy-coded data
        const int flips = 1 + rnd() % 6;
        for (int k = 0; k < flips; ++k) m[body + rnd() % (m.size() - body)] = (uint8_t)rnd();
      } else if (kind == 1) {   // truncation inside the scan
        m.resize(body + rnd() % (m.size() - body));
      } else if (kind == 2) {   // inserted markers
        const int ins = 1 + rnd() % 3;
        for (int k = 0; k < ins; ++k) { const size_t p = body + rnd() % (m.size() - body - 1); m[p] = 0xFF; m[p + 1] = (uint8_t)(0xD0 + rnd() % 16); }
      } else {                  // a run of 0xFF 0x00 pairs and of zeros: stuffing at subsequence boundaries, long codes
        const size_t p = body + rnd() % (m.size() - body - 40);
        for (int k = 0; k < 32; ++k) m[p + k] = (uint8_t)((rnd() & 1) ? ((k & 1) ? 0x00 : 0xFF) : 0x00);
      }
      if (run_one(m, kSubseq[rnd() % 4], kCaps[rnd() % 4])) return 3;
    }
  }
  printf("jpeg_sync_fuzz: %ld streams, %ld declined, %ld flagged\n", twin_runs, declined, flagged);
  return 0;
}
