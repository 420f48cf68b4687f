// jpeg.hip — image ingest: baseline JPEG -> RGB u8 on the device.
//
// Replaces read_image's file decode (detectors/_east/utils.py:477-497: cv2.imread / PIL, both libjpeg-turbo with its default
// decompression settings: JDCT_ISLOW, fancy upsampling, JFIF YCbCr -> RGB) for the formats a scanner / camera page comes in:
// 8-bit baseline or extended-sequential Huffman JPEG, grayscale or YCbCr with 4:4:4, 4:2:2 (h2v1) or 4:2:0 (h2v2) sampling,
// one interleaved scan, restart markers.  Anything else (progressive, arithmetic, CMYK, 12-bit, multi-scan, h1v2) is reported
// as unsupported and the caller falls back to the host decoder.
// Exif orientation (what cv2.imread / ImageOps.exif_transpose apply): msocr_jpeg_parse_host refuses a stream with orientation 2..8,
// msocr_jpeg_parse_oriented_host — the same marker walk — reports it, and msocr_jpeg_reconstruct_oriented applies it in the last
// write of the colour stage: mirrored destinations for 2..4 (jpeg_color_kernel<true>), a tiled transpose through LDS for 5..8
// (jpeg_color_transpose_kernel), so a portrait page photographed in landscape costs no extra pass over its pixels.
//
// Split: parsing runs on the HOST (msocr_jpeg_parse_host), and so does the serial Huffman decoder that judges every stream
// (msocr_jpeg_entropy_decode_host -> quantised DCT coefficients, 2 bytes each).  A stream WITH a restart interval (DRI) is a sequence
// of independent, byte-aligned bit streams (DC predictors reset at every RSTn): the host only walks the markers
// (msocr_jpeg_scan_prepare_host: interval bounds + Huffman tables), the file bytes go to the device as they are and ONE THREAD PER
// INTERVAL decodes them there (msocr_jpeg_entropy_decode_device).  A stream WITHOUT one, or an interval too long for one thread, is
// one serial bit stream: the self-synchronising stage (msocr_jpeg_entropy_decode_sync_device, below the per-interval kernel) cuts it
// into subsequences that are decoded in parallel from guessed states and brought into step in rounds.  Either way 0.3-1.6 MB of file
// bytes cross PCIe instead of 9.4 MB of coefficients per 2048 x 1536 page, and no host core decodes anything.  Everything per-pixel —
// dequantisation + inverse DCT, chroma upsampling, colour conversion — runs on the DEVICE (msocr_jpeg_reconstruct), so the
// page's pixels are produced in HBM and never cross PCIe.  The reconstruction arithmetic is libjpeg's, restated from its
// published algorithms (jidctint.c "islow" 13-bit fixed point, jdsample.c triangle-filter upsampling, jdcolor.c 16-bit YCC
// tables) in __host__ __device__ functions: msocr_jpeg_reconstruct_host runs the same code on the CPU, which is how the CPU
// test-suite pins it bit for bit against PIL's decode of the same files.
//
// Layout.  What every decoder shares comes first and exists once: the table (DevTable; HuffTable adds what it is built from), the
// symbol decoder (interval_symbol, templated on the bit reader), HUFF_EXTEND (extend), the coefficient address of a block
// (block_offset, mcu_block), an interval's MCU count (interval_mcus).  Then the host side: parse, the marker walk of an interval
// (interval_walk: the serial decoder's restart handling and scan_prepare's bounds), the serial decoder.  Then the per-interval
// decoder and its kernel (stage_tables puts a page's tables into LDS for every Huffman kernel), the self-synchronising stage,
// the reconstruction (reconstruct / reconstruct_host behind the upright and the oriented entries), and the C entries.
// Separate on purpose: the three bit readers and the serial decoder's loop (reasons beside four_plain_bytes and entropy_decode),
// the two hand-written block scans (a plain sum in jpeg_sync_place_kernel, a segmented one in jpeg_sync_dc_kernel), and the
// transposing colour kernel (its workgroup owns a tile, not a run of pixels).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "internal.h"
#include "msocr.h"

#define HD __host__ __device__ __forceinline__

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---------------------------------------------------------------------------------------------------- shared by every decoder
// The lookup arrays of one Huffman table: what a decoder reads, on the host and (as part of a ScanDesc, staged into LDS) on the
// device; 1420 bytes.
struct DevTable {
  uint16_t look[512];   // fast path: 9-bit lookahead -> (length << 8) | symbol, 0 = longer code
  int32_t maxcode[18];  // largest code of each length (-1 none), [17] = sentinel
  int32_t valoff[17];
  uint8_t vals[256];
};

// One Huffman symbol from any of the three bit readers (peek(n) = the next n bits, filled by the caller or on demand; skip(n)).
// -1: no code of up to 16 bits matches.
template <class Bits>
HD int interval_symbol(Bits& br, const DevTable& t) {
  const uint32_t look = br.peek(9);
  const uint32_t e = t.look[look];
  if (e) { br.skip((int)(e >> 8)); return (int)(e & 0xff); }
  int l = 9;
  int32_t code;
  for (;;) {  // codes longer than 9 bits
    ++l;
    if (l > 16) return -1;
    code = (int32_t)br.peek(l);
    if (t.maxcode[l] >= 0 && code <= t.maxcode[l]) break;
  }
  br.skip(l);
  return t.vals[(code + t.valoff[l]) & 0xff];
}
HD int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }  // HUFF_EXTEND

// Coefficient offset of block (by, bx) of MCU (my, mx) in component c's plane of blocks.
HD int64_t block_offset(const msocr_jpeg_info& f, int c, int my, int mx, int by, int bx) {
  return f.coef_off[c] + ((int64_t)(my * f.vs[c] + by) * f.blocks_w[c] + (mx * f.hs[c] + bx)) * 64;
}
// Block b of an interleaved MCU (the nb0 = hs[0] * vs[0] luma blocks row by row, then Cb, then Cr; a grey MCU is one block)
// -> its component, *by / *bx = where it sits in that component's part of the MCU.
HD int mcu_block_comp(const msocr_jpeg_info& f, int nb0, int b) { return f.ncomp == 1 ? 0 : (b < nb0 ? 0 : b - nb0 + 1); }
HD int mcu_block(const msocr_jpeg_info& f, int nb0, int b, int* by, int* bx) {
  const int c = mcu_block_comp(f, nb0, b);
  *by = c == 0 ? b / f.hs[0] : 0;
  *bx = c == 0 ? b - *by * f.hs[0] : 0;
  return c;
}
// MCUs of the restart interval that starts at MCU `first` of `total`.
HD int interval_mcus(int total, int restart_interval, int first) {
  return total - first < restart_interval ? total - first : restart_interval;
}
// The step the two device bit readers share: four stream bytes (little-endian load) hold no 0xFF, i.e. no stuffing and no marker
// -> *be = the four in stream order.  The readers stay three (BitReader fills on demand and stops at a marker, IntervalBits
// un-stuffs five bytes in registers, SyncBits tracks file bit positions): each sits in a hot loop shaped for it.
HD bool four_plain_bytes(uint32_t lo, uint32_t* be) {
  if ((((~lo) - 0x01010101u) & lo & 0x80808080u) != 0) return false;
  *be = (lo << 24) | ((lo & 0xff00u) << 8) | ((lo >> 8) & 0xff00u) | (lo >> 24);
  return true;
}

// ---------------------------------------------------------------------------------------------------- host: parse + Huffman
struct HuffTable {      // a DevTable and what it is built from
  DevTable lut = {};
  bool present = false;
  uint8_t bits[17] = {0};
  // false: the code lengths do not form a prefix code (libjpeg jdhuff.c jpeg_make_d_derived_tbl -> JERR_BAD_HUFF_TABLE)
  bool build() {
    int code = 0, k = 0;
    int32_t huffcode[256];
    uint8_t huffsize[256];
    for (int l = 1; l <= 16; ++l)
      for (int i = 0; i < bits[l]; ++i) { huffsize[k] = (uint8_t)l; ++k; }
    const int n = k;
    k = 0;
    int si = n ? huffsize[0] : 0;
    while (k < n) {
      while (k < n && huffsize[k] == si) huffcode[k++] = code++;
      if (code > (1 << si)) return false;  // over-subscribed at this length: more codes than si bits can hold
      code <<= 1;
      ++si;
    }
    int p = 0;
    for (int l = 1; l <= 16; ++l) {
      if (bits[l]) {
        lut.valoff[l] = p - huffcode[p];
        p += bits[l];
        lut.maxcode[l] = huffcode[p - 1];
      } else {
        lut.maxcode[l] = -1;
        lut.valoff[l] = 0;
      }
    }
    lut.maxcode[17] = 0x7fffffff;
    memset(lut.look, 0, sizeof(lut.look));
    p = 0;
    for (int l = 1; l <= 9; ++l)
      for (int i = 0; i < bits[l]; ++i, ++p) {
        const int base = huffcode[p] << (9 - l);
        if (base + (1 << (9 - l)) > 512) return false;  // unreachable after the check above; keeps the table write in bounds
        for (int c = 0; c < (1 << (9 - l)); ++c) lut.look[base + c] = (uint16_t)((l << 8) | lut.vals[p]);
      }
    return true;
  }
};

struct BitReader {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc = 0;
  int nbits = 0;
  bool hit_marker = false;
  void fill() {
    while (nbits <= 56) {
      int b = 0;
      if (!hit_marker && p < end) {
        b = *p;
        if (b == 0xFF) {
          if (p + 1 < end && p[1] == 0x00) p += 2;     // stuffed byte
          else { hit_marker = true; b = 0; }           // a marker: feed zeros (libjpeg does the same past the end of a segment)
        } else {
          ++p;
        }
      }
      acc = (acc << 8) | (uint64_t)b;
      nbits += 8;
    }
  }
  inline int peek(int n) { if (nbits < n) fill(); return (int)((acc >> (nbits - n)) & ((1u << n) - 1)); }
  inline void skip(int n) { nbits -= n; }
  inline int get(int n) { if (n == 0) return 0; const int v = peek(n); skip(n); return v; }
  void restart() { acc = 0; nbits = 0; hit_marker = false; }
};

struct Parsed {
  msocr_jpeg_info info;
  HuffTable dc[4], ac[4];
  int dc_sel[3], ac_sel[3];
  int restart_interval = 0;
  const uint8_t* scan = nullptr;  // first byte of the entropy-coded segment
  int mcus_x = 0, mcus_y = 0;
};

inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Largest frame taken (pixels): PIL refuses anything above 2 x MAX_IMAGE_PIXELS (DecompressionBombError), so the host
// decoder the caller falls back to gives the same answer; below it the coefficient array is at most 0.54 GB.
constexpr int64_t kMaxPixels = 2 * (int64_t)89478485;

// Exif Orientation (tag 0x0112 of IFD0) of an APP1 payload, 1 when absent / unreadable.
int exif_orientation(const uint8_t* s, int n) {
  if (n < 14 || memcmp(s, "Exif\0\0", 6) != 0) return 1;
  const uint8_t* t = s + 6;
  const int tn = n - 6;
  bool le;
  if (t[0] == 'I' && t[1] == 'I') le = true;
  else if (t[0] == 'M' && t[1] == 'M') le = false;
  else return 1;
  auto u16 = [&](int o) { return le ? (t[o] | (t[o + 1] << 8)) : ((t[o] << 8) | t[o + 1]); };
  auto u32 = [&](int o) {
    return le ? ((uint32_t)t[o] | ((uint32_t)t[o + 1] << 8) | ((uint32_t)t[o + 2] << 16) | ((uint32_t)t[o + 3] << 24))
              : (((uint32_t)t[o] << 24) | ((uint32_t)t[o + 1] << 16) | ((uint32_t)t[o + 2] << 8) | (uint32_t)t[o + 3]);
  };
  if (u16(2) != 42) return 1;
  const uint32_t ifd = u32(4);
  if (ifd > (uint32_t)tn || (int64_t)ifd + 2 > tn) return 1;
  const int cnt = u16((int)ifd);
  for (int e = 0; e < cnt; ++e) {
    const int64_t o = (int64_t)ifd + 2 + 12 * (int64_t)e;
    if (o + 12 > tn) return 1;
    if (u16((int)o) == 0x0112) return (u16((int)o + 2) == 3 && u32((int)o + 4) == 1) ? u16((int)o + 8) : 1;
  }
  return 1;
}

// What the marker walk does with an Exif APP1 segment.
enum ExifRule {
  kExifRefuse,   // msocr_jpeg_parse_host: a stream with orientation 2..8 is not the upright reconstruction's
  kExifReport,   // msocr_jpeg_parse_oriented_host: the orientation is returned; two Exif segments are the host reader's to judge
  kExifIgnore    // the re-parse inside the entropy entries: `info` comes from one of the two above, which has judged the segment
};

// Walks the markers up to the first SOS.  Returns MSOCR_OK, or MSOCR_E_ARG for a corrupt / unsupported stream.
// *orientation (kExifReport) = 1..8.
int parse(const uint8_t* d, int64_t len, Parsed* P, ExifRule exif = kExifRefuse, int32_t* orientation = nullptr) {
  memset(&P->info, 0, sizeof(P->info));
  if (orientation) *orientation = 1;
  int exif_segments = 0;
  if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) return MSOCR_E_ARG;
  uint16_t qt[4][64];
  bool qt_present[4] = {false, false, false, false};
  int qsel[3] = {0, 0, 0}, comp_id[3] = {0, 0, 0};
  bool have_sof = false, adobe = false;
  int adobe_transform = -1;
  int64_t i = 2;
  while (i + 4 <= len) {
    if (d[i] != 0xFF) return MSOCR_E_ARG;
    while (i < len && d[i] == 0xFF) ++i;  // fill bytes
    if (i >= len) return MSOCR_E_ARG;
    const int m = d[i++];
    if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
    if (m == 0xD9) return MSOCR_E_ARG;
    if (i + 2 > len) return MSOCR_E_ARG;
    const int L = rd16(d + i);
    if (L < 2 || i + L > len) return MSOCR_E_ARG;
    const uint8_t* s = d + i + 2;
    const int n = L - 2;
    if (m == 0xDB) {  // DQT
      int o = 0;
      while (o < n) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        ++o;
        if (tq > 3 || pq > 1 || o + 64 * (pq + 1) > n) return MSOCR_E_ARG;
        for (int k = 0; k < 64; ++k) {
          qt[tq][kZigzag[k]] = pq ? (uint16_t)rd16(s + o + 2 * k) : s[o + k];
        }
        o += 64 * (pq + 1);
        qt_present[tq] = true;
      }
    } else if (m == 0xC4) {  // DHT
      int o = 0;
      while (o < n) {
        if (o + 17 > n) return MSOCR_E_ARG;
        const int tc = s[o] >> 4, th = s[o] & 15;
        if (tc > 1 || th > 3) return MSOCR_E_ARG;
        HuffTable& t = tc ? P->ac[th] : P->dc[th];
        int cnt = 0;
        t.bits[0] = 0;
        for (int l = 1; l <= 16; ++l) { t.bits[l] = s[o + l]; cnt += t.bits[l]; }
        o += 17;
        if (cnt > 256 || o + cnt > n) return MSOCR_E_ARG;
        memcpy(t.lut.vals, s + o, cnt);
        o += cnt;
        t.present = true;
        if (!t.build()) return MSOCR_E_ARG;
      }
    } else if (m == 0xC0 || m == 0xC1) {  // SOF0 / SOF1: baseline / extended sequential, Huffman
      if (n < 6 || have_sof) return MSOCR_E_ARG;
      if (s[0] != 8) return MSOCR_E_ARG;
      P->info.height = rd16(s + 1);
      P->info.width = rd16(s + 3);
      P->info.ncomp = s[5];
      if (P->info.height <= 0 || P->info.width <= 0 || (P->info.ncomp != 1 && P->info.ncomp != 3) || n < 6 + 3 * P->info.ncomp)
        return MSOCR_E_ARG;
      if ((int64_t)P->info.height * P->info.width > kMaxPixels) return MSOCR_E_ARG;
      for (int c = 0; c < P->info.ncomp; ++c) {
        comp_id[c] = s[6 + 3 * c];
        P->info.hs[c] = s[7 + 3 * c] >> 4;
        P->info.vs[c] = s[7 + 3 * c] & 15;
        qsel[c] = s[8 + 3 * c];
        if (qsel[c] > 3) return MSOCR_E_ARG;
      }
      have_sof = true;
    } else if ((m >= 0xC2 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      return MSOCR_E_ARG;  // progressive / lossless / arithmetic / hierarchical: host decoder
    } else if (m == 0xDD) {
      if (n < 2) return MSOCR_E_ARG;
      P->restart_interval = rd16(s);
    } else if (m == 0xE1 && exif != kExifIgnore) {
      // cv2.imread (the reference's read_image) applies the Exif orientation, and so does read_image here.  The upright
      // reconstruction does not rotate: under kExifRefuse such files go to the host decoder; under kExifReport the caller gets
      // the orientation and reconstructs with msocr_jpeg_reconstruct_oriented.
      const int orient = exif_orientation(s, n);
      const bool turned = orient >= 2 && orient <= 8;
      if (exif == kExifRefuse) {
        if (turned) return MSOCR_E_ARG;
      } else if (n >= 6 && memcmp(s, "Exif\0\0", 6) == 0) {
        if (++exif_segments > 1) return MSOCR_E_ARG;  // PIL and cv2 differ on which segment wins
        if (orientation && turned) *orientation = orient;
      }
    } else if (m == 0xEE && n >= 12 && memcmp(s, "Adobe", 5) == 0) {
      adobe = true;
      adobe_transform = s[11];
    } else if (m == 0xDA) {  // SOS
      if (!have_sof || n < 1) return MSOCR_E_ARG;
      const int ns = s[0];
      if (ns != P->info.ncomp || n < 1 + 2 * ns + 3) return MSOCR_E_ARG;  // one interleaved scan with every component
      for (int k = 0; k < ns; ++k) {
        int c = -1;
        for (int q = 0; q < P->info.ncomp; ++q)
          if (comp_id[q] == s[1 + 2 * k]) c = q;
        if (c != k) return MSOCR_E_ARG;  // scan order = frame order (what every baseline encoder writes)
        P->dc_sel[c] = s[2 + 2 * k] >> 4;
        P->ac_sel[c] = s[2 + 2 * k] & 15;
        if (P->dc_sel[c] > 3 || P->ac_sel[c] > 3 || !P->dc[P->dc_sel[c]].present || !P->ac[P->ac_sel[c]].present) return MSOCR_E_ARG;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return MSOCR_E_ARG;
      P->scan = d + i + L;
      break;
    }
    i += L;
  }
  if (!P->scan) return MSOCR_E_ARG;
  msocr_jpeg_info& f = P->info;
  if (f.ncomp == 3) {
    // colour space as libjpeg decides it (jdapimin.c default_decompress_parms): Adobe transform 0 = RGB / ids 'R','G','B' = RGB
    if (adobe && adobe_transform == 0) return MSOCR_E_ARG;
    if (!adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return MSOCR_E_ARG;
    if (f.hs[1] != 1 || f.vs[1] != 1 || f.hs[2] != 1 || f.vs[2] != 1) return MSOCR_E_ARG;
    if (!((f.hs[0] == 1 && f.vs[0] == 1) || (f.hs[0] == 2 && f.vs[0] == 1) || (f.hs[0] == 2 && f.vs[0] == 2))) return MSOCR_E_ARG;
  } else {
    f.hs[0] = f.vs[0] = 1;  // a single-component scan is non-interleaved: one block per MCU whatever the sampling factors say
  }
  const int hmax = f.hs[0], vmax = f.vs[0];
  P->mcus_x = (f.width + 8 * hmax - 1) / (8 * hmax);
  P->mcus_y = (f.height + 8 * vmax - 1) / (8 * vmax);
  int64_t off = 0;
  for (int c = 0; c < f.ncomp; ++c) {
    if (!qt_present[qsel[c]]) return MSOCR_E_ARG;
    for (int k = 0; k < 64; ++k) f.quant[c][k] = qt[qsel[c]][k];
    f.blocks_w[c] = P->mcus_x * f.hs[c];
    f.blocks_h[c] = P->mcus_y * f.vs[c];
    f.coef_off[c] = off;
    off += (int64_t)f.blocks_w[c] * f.blocks_h[c] * 64;
  }
  f.coef_total = off;
  f.supported = 1;
  return MSOCR_OK;
}

// `info` of an entropy entry must be what a parse entry returned for this stream: parses it again (the Exif segment was judged
// then) and compares.
int reparse(const uint8_t* d, int64_t len, const msocr_jpeg_info* info, Parsed* P) {
  if (!info || parse(d, len, P, kExifIgnore) != MSOCR_OK) return MSOCR_E_ARG;
  const msocr_jpeg_info& f = P->info;
  return f.width == info->width && f.height == info->height && f.ncomp == info->ncomp && f.coef_total == info->coef_total ? MSOCR_OK
                                                                                                                        : MSOCR_E_ARG;
}

// The marker walk of one restart interval whose data starts at (or, for a reader that has consumed some, holds) `p`: *data_end =
// the first 0xFF that is not followed by a stuffed 0x00 (`end` when there is none) — where the interval's bits end; returns the
// byte behind the first RSTn at or after it — where the next interval starts — or nullptr when no RSTn follows.
const uint8_t* interval_walk(const uint8_t* p, const uint8_t* end, const uint8_t** data_end) {
  const uint8_t* e = p;
  for (;;) {
    e = e < end ? static_cast<const uint8_t*>(memchr(e, 0xFF, (size_t)(end - e))) : nullptr;
    if (!e) { e = end; break; }
    if (e + 1 < end && e[1] == 0x00) { e += 2; continue; }
    break;
  }
  *data_end = e;
  const uint8_t* q = e;
  while (q + 1 < end && !(q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7)) ++q;
  return q + 1 < end ? q + 2 : nullptr;
}

// The serial decoder: the host pool's product path and the judge of every stream.  It shares the table, the symbol decoder, the
// block addressing and the marker walk with the device decoders but keeps its own loop: decode_interval's one-symbol-per-
// iteration form (made for converged lanes) is slower on a host core (1.62 MB 4:2:0 page, one core: 17.6-18.5 ms against
// 20.6-21.2 ms through the per-interval host twin; 3.2 MB 4:4:4: 36.5-37.2 against 42.3-42.8 ms).
int entropy_decode(const Parsed& P, const uint8_t* end, int16_t* coef) {
  const msocr_jpeg_info& f = P.info;
  memset(coef, 0, sizeof(int16_t) * (size_t)f.coef_total);
  BitReader br;
  br.p = P.scan;
  br.end = end;
  int pred[3] = {0, 0, 0};
  int until_restart = P.restart_interval;
  for (int my = 0; my < P.mcus_y; ++my)
    for (int mx = 0; mx < P.mcus_x; ++mx) {
      if (P.restart_interval && until_restart == 0) {
        // byte-align, expect RSTn (br.p has not passed the interval's marker: the walk from it ends where the walk from the
        // interval's first byte does)
        br.restart();
        const uint8_t* data_end;
        br.p = interval_walk(br.p, end, &data_end);
        if (!br.p) return MSOCR_E_ARG;
        pred[0] = pred[1] = pred[2] = 0;
        until_restart = P.restart_interval;
      }
      for (int c = 0; c < f.ncomp; ++c) {
        const DevTable& dct = P.dc[P.dc_sel[c]].lut;
        const DevTable& act = P.ac[P.ac_sel[c]].lut;
        for (int by = 0; by < f.vs[c]; ++by)
          for (int bx = 0; bx < f.hs[c]; ++bx) {
            int16_t* blk = coef + block_offset(f, c, my, mx, by, bx);
            int s = interval_symbol(br, dct);
            if (s < 0 || s > 15) return MSOCR_E_ARG;
            if (s) pred[c] = (int)((uint32_t)pred[c] + (uint32_t)extend(br.get(s), s));  // modulo 2^32: a hostile stream wraps
            blk[0] = (int16_t)pred[c];
            for (int k = 1; k < 64;) {
              const int rs = interval_symbol(br, act);
              if (rs < 0) return MSOCR_E_ARG;
              const int r = rs >> 4, sz = rs & 15;
              if (sz == 0) {
                if (r != 15) break;  // EOB
                k += 16;
                continue;
              }
              k += r;
              if (k > 63) return MSOCR_E_ARG;
              blk[kZigzag[k]] = (int16_t)extend(br.get(sz), sz);
              ++k;
            }
          }
      }
      if (P.restart_interval) --until_restart;
    }
  return MSOCR_OK;
}

// ---------------------------------------------------------------------------------------------------- entropy decode per interval
// The decoder of ONE restart interval as a __host__ __device__ function: jpeg_huffman_kernel runs it one interval per thread,
// msocr_jpeg_entropy_decode_intervals_host runs the same code interval after interval on the CPU (how the CPU suite pins it against
// entropy_decode above and against PIL).  Same arithmetic and the same treatment of bad streams as entropy_decode: zeros are fed
// past the end of the interval (= at its marker), an undecodable code / a coefficient index past 63 is an error for the whole page.
struct ScanDesc {            // one page; msocr_jpeg_scan_desc_bytes() bytes, opaque to callers
  msocr_jpeg_info info;
  int64_t bytes_base;        // where the file's first byte sits in the batch byte buffer (the interval bounds are relative to the FILE)
  int32_t restart_interval, mcus_x, mcus_y, n_intervals;
  DevTable dc[3], ac[3];     // per component (duplicates when components share a table)
  uint8_t zigzag[64];
};

struct IntervalBits {
  const uint8_t* base;
  uint32_t pos, end;
  uint64_t acc;
  int nbits;
  // at least 33 valid bits afterwards (a code of up to 16 bits + up to 15 value bits per symbol)
  HD void refill() {
    if (nbits > 32) return;
    if (pos + 5 <= end) {
      // four stream bytes + one of lookahead, un-stuffed in registers: a lane that meets a 0xFF takes no memory round trips, so a
      // wave whose lanes are at different places of different streams pays the same few ALU instructions either way
      const uint64_t w = (uint64_t)base[pos] | ((uint64_t)base[pos + 1] << 8) | ((uint64_t)base[pos + 2] << 16) |
                         ((uint64_t)base[pos + 3] << 24) | ((uint64_t)base[pos + 4] << 32);
      uint32_t be;
      if (four_plain_bytes((uint32_t)w, &be)) {
        acc = (acc << 32) | (uint64_t)be;
        nbits += 32;
        pos += 4;
        return;
      }
      uint32_t i = 0;
      bool marker = false;
#pragma unroll
      for (int step = 0; step < 4; ++step) {
        if (!marker && i < 4) {
          const uint32_t b = (uint32_t)(w >> (8 * i)) & 0xff, n = (uint32_t)(w >> (8 * i + 8)) & 0xff;
          if (b != 0xFF) { acc = (acc << 8) | b; nbits += 8; i += 1; }
          else if (n == 0) { acc = (acc << 8) | 0xFF; nbits += 8; i += 2; }   // stuffed byte
          else marker = true;                                                 // zeros from here on
        }
      }
      pos += i;
      if (marker) end = pos;
      if (nbits > 32) return;
    }
    while (nbits <= 56) {
      uint32_t b = 0;
      if (pos < end) {
        b = base[pos];
        if (b == 0xFF) {
          if (pos + 1 < end && base[pos + 1] == 0x00) pos += 2;   // stuffed byte
          else { b = 0; end = pos; }                              // a marker: zeros from here on
        } else {
          ++pos;
        }
      }
      acc = (acc << 8) | (uint64_t)b;
      nbits += 8;
    }
  }
  HD uint32_t peek(int n) const { return (uint32_t)(acc >> (nbits - n)) & ((1u << n) - 1u); }
  HD void skip(int n) { nbits -= n; }
};

// One Huffman symbol per loop iteration, the same instruction sequence for a DC difference and an AC run/size: the 64 lanes of a
// wave decode 64 different intervals and stay converged except in the rare slow paths (codes longer than 9 bits, 0xFF bytes).
// `coef` = the page's zero-filled coefficient array.  Returns 0, or 1 for a bad stream.
HD int decode_interval(const msocr_jpeg_info& f, int mcus_x, const DevTable* dc, const DevTable* ac, const uint8_t* zigzag,
                       const uint8_t* bytes, uint32_t begin, uint32_t end, int first_mcu, int n_mcu, int16_t* coef) {
  IntervalBits br;
  br.base = bytes; br.pos = begin; br.end = end; br.acc = 0; br.nbits = 0;
  const int nb0 = f.hs[0] * f.vs[0];
  const int per_mcu = f.ncomp == 3 ? nb0 + 2 : 1;
  int pred0 = 0, pred1 = 0, pred2 = 0;
  int mcu = first_mcu, b = 0, k = 0, c = 0;
  int my = mcu / mcus_x, mx = mcu - my * mcus_x;
  int64_t blk = block_offset(f, 0, my, mx, 0, 0);
  const int last = first_mcu + n_mcu;
  while (mcu < last) {
    br.refill();
    const int sym = interval_symbol(br, k == 0 ? dc[c] : ac[c]);
    if (sym < 0) return 1;
    const int sz = k == 0 ? sym : (sym & 15);
    if (k == 0 && sz > 15) return 1;
    int v = 0;
    if (sz) {
      v = (int)br.peek(sz);
      br.skip(sz);
      v = extend(v, sz);
    }
    if (k == 0) {
      int pr = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
      pr = (int)((uint32_t)pr + (uint32_t)v);
      if (c == 0) pred0 = pr; else if (c == 1) pred1 = pr; else pred2 = pr;
      coef[blk] = (int16_t)pr;
      k = 1;
    } else {
      const int r = sym >> 4;
      if (sz == 0) {
        k = r == 15 ? k + 16 : 64;          // ZRL / EOB
      } else {
        k += r;
        if (k > 63) return 1;
        coef[blk + zigzag[k]] = (int16_t)v;
        ++k;
      }
    }
    if (k >= 64) {                          // next block of the MCU / next MCU
      k = 0;
      if (++b == per_mcu) {
        b = 0;
        ++mcu;
        if (++mx == mcus_x) { mx = 0; ++my; }
      }
      int by, bx;
      c = mcu_block(f, nb0, b, &by, &bx);
      blk = block_offset(f, c, my, mx, by, bx);
    }
  }
  return 0;
}

// The page's six tables and the zigzag order -> LDS, by all THREADS threads of the workgroup (ends with the barrier).
template <int THREADS>
__device__ __forceinline__ void stage_tables(const ScanDesc& d, DevTable* s_dc, DevTable* s_ac, uint8_t* s_zz) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(d.dc);
  uint32_t* d0 = reinterpret_cast<uint32_t*>(s_dc);
  uint32_t* d1 = reinterpret_cast<uint32_t*>(s_ac);
  constexpr int W = (int)(3 * sizeof(DevTable) / 4);
  for (int i = threadIdx.x; i < W; i += THREADS) { d0[i] = src[i]; d1[i] = src[W + i]; }
  if (THREADS == 64 || threadIdx.x < 64) s_zz[threadIdx.x] = d.zigzag[threadIdx.x];
  __syncthreads();
}

// One wave = `lanes` consecutive intervals of ONE page (blockIdx.y); the page's six tables sit in LDS (all 64 threads load them).
// lanes < 64 when the batch has fewer intervals than the chip has wave slots: the decoder is a chain of dependent instructions, a
// lane costs the same whether its 63 neighbours work or not, and a wave executes the UNION of its lanes' slow paths (a 0xFF byte,
// a code longer than 9 bits) — so few intervals are spread one per wave over the 1024 SIMDs instead of packed into 32 waves
// (16 pages x 128 intervals: 22.7 ms packed).
__global__ __launch_bounds__(64) void jpeg_huffman_kernel(const uint8_t* __restrict__ bytes, const ScanDesc* __restrict__ descs,
                                                          const uint32_t* __restrict__ bounds, const int64_t* __restrict__ page_base,
                                                          int16_t* __restrict__ coef, int32_t* __restrict__ status, int lanes) {
  __shared__ DevTable s_dc[3], s_ac[3];
  __shared__ uint8_t s_zz[64];
  const ScanDesc& d = descs[blockIdx.y];
  if ((int)blockIdx.x * lanes >= d.n_intervals) return;    // uniform
  stage_tables<64>(d, s_dc, s_ac, s_zz);
  const int iv = blockIdx.x * lanes + threadIdx.x;
  if ((int)threadIdx.x >= lanes || iv >= d.n_intervals) return;
  const int64_t coef_base = page_base[2 * blockIdx.y], first_interval = page_base[2 * blockIdx.y + 1];
  const uint32_t begin = bounds[2 * (first_interval + iv)], end = bounds[2 * (first_interval + iv) + 1];
  const int first = iv * d.restart_interval;
  if (decode_interval(d.info, d.mcus_x, s_dc, s_ac, s_zz, bytes + d.bytes_base, begin, end, first,
                      interval_mcus(d.mcus_x * d.mcus_y, d.restart_interval, first), coef + coef_base))
    status[blockIdx.y] = 1;
}

// ---------------------------------------------------------------------------------------------------- self-synchronising decode
// ONE serial entropy-coded segment (a stream without DRI, or one long restart interval) decoded in parallel.  The interval's bytes
// are cut into subsequences of S bytes, one thread each.  A decoder state at a symbol boundary is (bit position in the file, block
// inside the MCU, zigzag index k); the DC predictors are not part of it: the write pass stores DC DIFFERENCES and a prefix sum per
// component turns them into values afterwards.  The first subsequence of an interval starts in the true state, every other one
// from a guess; a Huffman decoder in a wrong state falls into step with the true decode after a short distance, so
//   rounds  : every subsequence is decoded (nothing written) from its entry state to the first symbol that starts behind its last
//             byte and leaves that exit state and the number of blocks it completed; in the next round it takes its predecessor's
//             exit state as entry state and decodes again if that differs from what it used.  Fixed point: entry[i] == exit[i-1]
//             for all i; subsequence r is final after round r, self-synchronisation makes it a handful of rounds instead of N.
//             Rounds are kernel launches (their order on the stream is the only ordering between workgroups); exit states are
//             double-buffered so that a round reads only what the round before wrote, and a page where a round changed nothing
//             returns at once from every later round.
//   place   : exclusive prefix sum of the block counts -> the first block of every subsequence.
//   write   : every subsequence is decoded once more from its final entry state and scatters its coefficients.  This pass IS the
//             decode along the true chain of states, so it alone judges the stream (status 1); what a speculative decode meets
//             (undecodable codes, DC sizes > 15, k > 63, all the time) only makes an exit state that is not valid yet.
//   dc      : per component, segmented inclusive prefix sum of the differences in scan order, modulo 2^16 (= the serial decoder's
//             (int16_t) of its modulo-2^32 predictor).
// The same __host__ __device__ functions run in the kernels and in msocr_jpeg_entropy_decode_sync_host.
constexpr uint32_t kSyncTailBlocks = 64;   // blocks one thread may decode from the zeros behind the data's end (<= 64 symbols each)

struct SyncBits {          // IntervalBits that knows where in the FILE its next unread bit sits
  const uint8_t* base;
  uint32_t pos, end;       // next byte to load (runs on past `end`: virtual zero bytes, so that positions stay monotonic)
  uint64_t acc;
  int nbits;
  uint32_t stuffed;        // bit j: the byte loaded j loads ago was a 0xFF, i.e. took two file bytes
  HD void load_byte() {
    uint32_t b = 0, ff = 0;
    if (pos < end) { b = base[pos]; ff = b == 0xFF; }
    pos += 1 + ff;         // [begin, end) of an interval holds no marker: a 0xFF in it is followed by its stuffed 0x00
    acc = (acc << 8) | (uint64_t)b;
    stuffed = (stuffed << 1) | ff;
    nbits += 8;
  }
  // at least 33 valid bits afterwards
  HD void refill() {
    if (nbits > 32) return;
    if (pos + 4 <= end) {
      const uint32_t lo = (uint32_t)base[pos] | ((uint32_t)base[pos + 1] << 8) | ((uint32_t)base[pos + 2] << 16) | ((uint32_t)base[pos + 3] << 24);
      uint32_t be;
      if (four_plain_bytes(lo, &be)) {
        acc = (acc << 32) | (uint64_t)be;
        nbits += 32;
        pos += 4;
        stuffed <<= 4;
        return;
      }
    }
    while (nbits <= 32) load_byte();
  }
  HD void start(const uint8_t* b, uint32_t bit, uint32_t e) {
    base = b; pos = bit >> 3; end = e; acc = 0; nbits = 0; stuffed = 0;
    load_byte();
    nbits -= (int)(bit & 7);
  }
  HD uint32_t peek(int n) const { return (uint32_t)(acc >> (nbits - n)) & ((1u << n) - 1u); }
  HD void skip(int n) { nbits -= n; }
  // File bit position of the next unread bit.  A stuffed 0x00 counts as read together with its 0xFF, so a position never points into
  // one and the same place in the stream always gives the same number, however much was buffered.
  HD uint32_t bitpos() const {
    const int nb = (nbits + 7) >> 3;                                   // buffered bytes with an unread bit, <= 8
    const uint32_t m = stuffed & ((1u << nb) - 1u);
#ifdef __HIP_DEVICE_COMPILE__
    const int ns = __popc(m);
#else
    const int ns = __builtin_popcount(m);
#endif
    return pos * 8u - (uint32_t)nbits - 8u * (uint32_t)ns;
  }
};

HD uint64_t sync_pack(uint32_t bit, int b, int k) { return (uint64_t)bit | ((uint64_t)(uint32_t)b << 32) | ((uint64_t)(uint32_t)k << 40); }

// Decodes symbols from `state` on.  Count mode: every symbol that starts before bit `stop`; *n_out = blocks completed.  Write mode:
// the same symbols (and, with `tail`, on into the zeros behind the data) as long as the block they belong to — number `blk` of the
// interval — is one of the interval's `need` blocks: that is what keeps every coefficient address inside the page's array.  The two
// modes treat what a valid stream cannot hold in the same way (an undecodable code = 16 bits skipped, symbol 0; a DC size > 15 =
// its low four bits; k > 63 = end of block), so their state sequences are the same; only write mode reports it (*bad).
// Every iteration consumes at least one bit: bounded by the bytes of the subsequence, the tail by kSyncTailBlocks * 64 symbols.
// Returns the state at the first symbol not decoded.
template <bool WRITE>
HD uint64_t sync_decode(const ScanDesc& d, const DevTable* dc, const DevTable* ac, const uint8_t* zigzag, const uint8_t* bytes,
                        uint32_t end, uint64_t state, uint32_t stop, bool tail, uint32_t blk, uint32_t need, int first_mcu,
                        int16_t* coef, uint32_t* n_out, int* bad) {
  const msocr_jpeg_info& f = d.info;
  SyncBits br;
  br.start(bytes, (uint32_t)state, end);
  int b = (int)((state >> 32) & 0xff), k = (int)((state >> 40) & 0xff);
  const int nb0 = f.hs[0] * f.vs[0];
  const int per_mcu = f.ncomp == 3 ? nb0 + 2 : 1;
  uint32_t n = 0, at;
  int mx = 0, my = 0, bb = 0;
  int64_t addr = 0;
  auto block_addr = [&]() {
    int by, bx;
    const int c = mcu_block(f, nb0, bb, &by, &bx);
    return block_offset(f, c, my, mx, by, bx);
  };
  if (WRITE) {
    const int mcu = first_mcu + (int)(blk / (uint32_t)per_mcu);
    bb = (int)(blk % (uint32_t)per_mcu);
    my = mcu / d.mcus_x;
    mx = mcu - my * d.mcus_x;
    addr = block_addr();
  }
  for (;;) {
    br.refill();
    at = br.bitpos();
    if (WRITE ? (blk >= need || (at >= stop && !tail)) : at >= stop) break;
    int c = mcu_block_comp(f, nb0, b);
    c = c > 2 ? 2 : c;                                   // a guessed state may name a block no MCU has
    const bool is_dc = k == 0;
    int sym = interval_symbol(br, is_dc ? dc[c] : ac[c]);
    bool err = false;
    if (sym < 0) { br.skip(16); sym = 0; err = true; }
    if (is_dc && sym > 15) err = true;
    const int sz = sym & 15;
    int v = 0;
    if (sz) {
      v = (int)br.peek(sz);
      br.skip(sz);
      v = extend(v, sz);
    }
    if (is_dc) {
      if (WRITE) coef[addr] = (int16_t)v;                // the difference; jpeg_sync_dc_kernel sums
      k = 1;
    } else {
      const int r = sym >> 4;
      if (sz == 0) {
        k = r == 15 ? k + 16 : 64;                       // ZRL / EOB
      } else {
        k += r;
        if (k > 63) { err = true; k = 64; }
        else { if (WRITE) coef[addr + zigzag[k]] = (int16_t)v; ++k; }
      }
    }
    if (WRITE && err) *bad = 1;
    if (k >= 64) {                                       // next block of the MCU / next MCU
      k = 0;
      ++n;
      if (++b >= per_mcu) b = 0;
      if (WRITE) {
        ++blk;
        if (++bb == per_mcu) {
          bb = 0;
          if (++mx == d.mcus_x) { mx = 0; ++my; }
        }
        if (blk < need) addr = block_addr();
      }
    }
  }
  if (n_out) *n_out = n;
  return sync_pack(at, b, k);
}

struct SyncSub {                  // where subsequence i of a page sits
  uint32_t begin, end;            // its interval's data (file offsets; `end` = the first marker)
  uint32_t lo, stop;              // its first byte; symbols that start before bit `stop` are its own
  uint32_t first_sub, next_sub;   // the interval's first subsequence, the next interval's first subsequence
  uint32_t need;                  // blocks of the interval
  int first_mcu;
  bool first, last;
};

// bounds / sub_first: the PAGE's interval pairs and first-subsequence indices.  Every loop bounded by n_intervals.
HD SyncSub sync_locate(const ScanDesc& d, const uint32_t* bounds, const uint32_t* sub_first, uint32_t nsub, uint32_t S, uint32_t i) {
  int lo = 0, hi = d.n_intervals - 1;
  while (lo < hi) {                                      // last interval whose first subsequence is <= i
    const int mid = (lo + hi + 1) >> 1;
    if (sub_first[mid] <= i) lo = mid; else hi = mid - 1;
  }
  SyncSub q;
  q.first_sub = sub_first[lo];
  q.next_sub = lo + 1 < d.n_intervals ? sub_first[lo + 1] : nsub;
  q.begin = bounds[2 * lo];
  q.end = bounds[2 * lo + 1];
  q.first = i == q.first_sub;
  q.last = i + 1 == q.next_sub;
  const uint64_t from = (uint64_t)q.begin + (uint64_t)(i - q.first_sub) * S;
  q.lo = from < q.end ? (uint32_t)from : q.end;
  q.stop = (q.last || from + S > q.end ? q.end : (uint32_t)(from + S)) * 8u;
  const int per_mcu = d.info.ncomp == 3 ? d.info.hs[0] * d.info.vs[0] + 2 : 1;
  q.first_mcu = lo * d.restart_interval;
  const int n_mcu = interval_mcus(d.mcus_x * d.mcus_y, d.restart_interval, q.first_mcu);
  q.need = n_mcu > 0 ? (uint32_t)n_mcu * (uint32_t)per_mcu : 0u;
  return q;
}

// One subsequence in one round.  entry / ex_in / ex_out / cnt: the page's arrays.  Returns 1 when it decoded again.
HD int sync_round(const ScanDesc& d, const DevTable* dc, const DevTable* ac, const uint8_t* zigzag, const uint8_t* bytes,
                  const uint32_t* bounds, const uint32_t* sub_first, uint32_t nsub, uint32_t S, uint32_t i, int round,
                  uint64_t* entry, const uint64_t* ex_in, uint64_t* ex_out, uint32_t* cnt) {
  const SyncSub q = sync_locate(d, bounds, sub_first, nsub, S, i);
  uint64_t e;
  if (round == 0) {
    // the true state at the head of an interval; elsewhere the first whole bit of the subsequence, (block 0, k 0) — behind the
    // stuffed 0x00 when the previous byte is a 0xFF
    uint32_t p = q.lo;
    if (!q.first && p > q.begin && p < q.end && bytes[p - 1] == 0xFF) ++p;
    e = sync_pack(p * 8u, 0, 0);
  } else {
    if (q.first || i == 0) { ex_out[i] = ex_in[i]; return 0; }
    e = ex_in[i - 1];
    if (e == entry[i]) { ex_out[i] = ex_in[i]; return 0; }
  }
  entry[i] = e;
  uint32_t n = 0;
  ex_out[i] = sync_decode<false>(d, dc, ac, zigzag, bytes, q.end, e, q.stop, false, 0, 0, 0, nullptr, &n, nullptr);
  cnt[i] = n;
  return 1;
}

// One subsequence in the write pass; P = the page's exclusive prefix sums of cnt (nsub + 1 entries).  Returns the page status this
// subsequence asks for: 0, 1 (the true chain met what a valid stream cannot hold) or 2 (the data ends with more than
// kSyncTailBlocks blocks of the interval outstanding: a truncated stream, left to the serial decoder).
HD int sync_write(const ScanDesc& d, const DevTable* dc, const DevTable* ac, const uint8_t* zigzag, const uint8_t* bytes,
                  const uint32_t* bounds, const uint32_t* sub_first, uint32_t nsub, uint32_t S, uint32_t i, const uint64_t* entry,
                  const uint32_t* P, int16_t* coef) {
  const SyncSub q = sync_locate(d, bounds, sub_first, nsub, S, i);
  if (q.first_sub > i || q.next_sub > nsub || q.next_sub <= i) return 1;   // not what the prepare step lays out
  const uint32_t base = P[q.first_sub], blk0 = P[i] - base, done = P[q.next_sub] - base;
  bool tail = false;
  if (q.last && done < q.need) {
    if (q.need - done > kSyncTailBlocks) return 2;
    tail = true;
  }
  if (blk0 >= q.need) return 0;
  int bad = 0;
  sync_decode<true>(d, dc, ac, zigzag, bytes, q.end, entry[i], q.stop, tail, blk0, q.need, q.first_mcu, coef, nullptr, &bad);
  return bad;
}

// rounds taken and the verdict "no fixed point" of one page: `changed` = the page's flag of every round
HD int sync_rounds_taken(const int32_t* changed, int stride, int max_rounds, uint32_t nsub, int* declined) {
  *declined = 0;
  for (int r = 1; r < max_rounds; ++r)
    if (changed[(int64_t)r * stride] == 0) return r;     // round r decoded nothing again: the fixed point stood after round r - 1
  if ((uint32_t)max_rounds < nsub) *declined = 1;        // (subsequence r is final after round r: max_rounds >= nsub needs no proof)
  return max_rounds;
}

// The DC scan of component c: bpm = its blocks per MCU, L = its blocks in scan order, seg = those of one restart interval (the
// predictor starts from 0 at every multiple of seg).
struct DcScan { uint32_t bpm, L, seg; };
HD DcScan sync_dc_scan(const ScanDesc& d, int c) {
  DcScan s;
  s.bpm = (uint32_t)(d.info.hs[c] * d.info.vs[c]);
  s.L = (uint32_t)(d.mcus_x * d.mcus_y) * s.bpm;
  s.seg = d.restart_interval > 0 ? (uint32_t)d.restart_interval * s.bpm : s.L;
  return s;
}
HD int64_t sync_dc_addr(const ScanDesc& d, int c, uint32_t e) {   // element e of component c in scan order -> its DC coefficient
  const msocr_jpeg_info& f = d.info;
  const uint32_t bpm = sync_dc_scan(d, c).bpm;   // asked for here, not handed down: 52 instead of 71 VGPRs in jpeg_sync_dc_kernel
  const uint32_t mcu = e / bpm, j = e - mcu * bpm;
  const int by = (int)(j / (uint32_t)f.hs[c]), bx = (int)j - by * f.hs[c];
  const int my = (int)(mcu / (uint32_t)d.mcus_x), mx = (int)mcu - my * d.mcus_x;
  return block_offset(f, c, my, mx, by, bx);
}

struct SyncWorkspace {
  uint64_t *entry, *ex[2];
  uint32_t *P, *cnt;
  int32_t* changed;
};
// byte offsets of the six arrays inside the workspace; returns its size
int64_t sync_layout(int64_t total_subseq, int32_t n_pages, int32_t max_rounds, int64_t off[6]) {
  int64_t o = 0;
  off[0] = o; o += 8 * total_subseq;                       // entry
  off[1] = o; o += 8 * total_subseq;                       // exit states, even rounds
  off[2] = o; o += 8 * total_subseq;                       // exit states, odd rounds
  off[3] = o; o += 4 * (total_subseq + n_pages);           // P: one more entry than subsequences per page
  off[4] = o; o += 4 * total_subseq;                       // cnt
  off[5] = o; o += 4 * (int64_t)max_rounds * n_pages;      // changed[round][page]
  return (o + 15) / 16 * 16;
}
SyncWorkspace sync_workspace(void* base, int64_t total_subseq, int32_t n_pages, int32_t max_rounds) {
  int64_t off[6];
  sync_layout(total_subseq, n_pages, max_rounds, off);
  uint8_t* p = static_cast<uint8_t*>(base);
  SyncWorkspace w;
  w.entry = reinterpret_cast<uint64_t*>(p + off[0]);
  w.ex[0] = reinterpret_cast<uint64_t*>(p + off[1]);
  w.ex[1] = reinterpret_cast<uint64_t*>(p + off[2]);
  w.P = reinterpret_cast<uint32_t*>(p + off[3]);
  w.cnt = reinterpret_cast<uint32_t*>(p + off[4]);
  w.changed = reinterpret_cast<int32_t*>(p + off[5]);
  return w;
}

struct SyncArgs {                 // what every kernel of the sequence takes
  const uint8_t* bytes;
  const ScanDesc* descs;
  const uint32_t *bounds, *sub_first;
  const int64_t* page_base;       // [n_pages][4]: coefficient base, first interval, first subsequence (batch-wide), subsequences
  uint32_t S;
  int32_t n_pages, max_rounds;
  SyncWorkspace w;
};

// grid (subsequences of the longest page / 256, pages)
__global__ __launch_bounds__(256) void jpeg_sync_round_kernel(SyncArgs a, int round) {
  __shared__ DevTable s_dc[3], s_ac[3];
  __shared__ uint8_t s_zz[64];
  const int pg = blockIdx.y;
  const int64_t* pb = a.page_base + 4 * pg;
  const uint32_t nsub = (uint32_t)pb[3];
  if (blockIdx.x * 256u >= nsub) return;                                        // uniform
  if (round >= 2 && a.w.changed[(int64_t)(round - 1) * a.n_pages + pg] == 0) return;   // uniform: the page stands
  const ScanDesc& d = a.descs[pg];
  stage_tables<256>(d, s_dc, s_ac, s_zz);
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nsub) return;
  const int64_t sb = pb[2];
  const int ch = sync_round(d, s_dc, s_ac, s_zz, a.bytes + d.bytes_base, a.bounds + 2 * pb[1], a.sub_first + pb[1], nsub, a.S, i, round,
                            a.w.entry + sb, a.w.ex[(round + 1) & 1] + sb, a.w.ex[round & 1] + sb, a.w.cnt + sb);
  if (ch && round >= 1) a.w.changed[(int64_t)round * a.n_pages + pg] = 1;
}

// one workgroup per page: exclusive prefix sum of cnt -> P (nsub + 1 entries per page, page p's at first subsequence + p), the
// rounds taken, and status 2 for a page whose rounds did not reach the fixed point
__global__ __launch_bounds__(256) void jpeg_sync_place_kernel(SyncArgs a, int32_t* __restrict__ status, int32_t* __restrict__ rounds) {
  __shared__ uint32_t s_sum[256];
  const int pg = blockIdx.x, tid = threadIdx.x;
  const int64_t* pb = a.page_base + 4 * pg;
  const uint32_t nsub = (uint32_t)pb[3];
  const uint32_t* cnt = a.w.cnt + pb[2];
  uint32_t* P = a.w.P + pb[2] + pg;
  if (tid == 0) {
    int declined;
    const int r = sync_rounds_taken(a.w.changed + pg, a.n_pages, a.max_rounds, nsub, &declined);
    if (rounds) rounds[pg] = r;
    if (declined) status[pg] = 2;
  }
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nsub; base += 2048) {
    uint32_t v[8], sum = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t i = base + tid * 8 + j;
      v[j] = i < nsub ? cnt[i] : 0;
      sum += v[j];
    }
    s_sum[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const uint32_t t = tid >= off ? s_sum[tid - off] : 0;
      __syncthreads();
      s_sum[tid] += t;
      __syncthreads();
    }
    uint32_t run = carry + s_sum[tid] - sum;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t i = base + tid * 8 + j;
      if (i < nsub) P[i] = run;
      run += v[j];
    }
    carry += s_sum[255];
    __syncthreads();
  }
  if (tid == 0) P[nsub] = carry;
}

__global__ __launch_bounds__(256) void jpeg_sync_write_kernel(SyncArgs a, int16_t* __restrict__ coef, int32_t* __restrict__ status) {
  __shared__ DevTable s_dc[3], s_ac[3];
  __shared__ uint8_t s_zz[64];
  const int pg = blockIdx.y;
  const int64_t* pb = a.page_base + 4 * pg;
  const uint32_t nsub = (uint32_t)pb[3];
  if (blockIdx.x * 256u >= nsub) return;            // uniform
  if (status[pg] == 2) return;                      // no fixed point (set by the place kernel, a launch ago): nothing to write
  const ScanDesc& d = a.descs[pg];
  stage_tables<256>(d, s_dc, s_ac, s_zz);
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nsub) return;
  const int st = sync_write(d, s_dc, s_ac, s_zz, a.bytes + d.bytes_base, a.bounds + 2 * pb[1], a.sub_first + pb[1], nsub, a.S, i,
                            a.w.entry + pb[2], a.w.P + pb[2] + pg, coef + pb[0]);
  if (st) atomicMax(&status[pg], st);
}

// grid (3 components, pages): segmented inclusive scan of the DC differences in scan order, 2048 elements per step, carried on
__global__ __launch_bounds__(256) void jpeg_sync_dc_kernel(SyncArgs a, int16_t* __restrict__ coef_all) {
  __shared__ uint32_t s_v[256], s_f[256];
  const int pg = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const ScanDesc& d = a.descs[pg];
  if (c >= d.info.ncomp) return;
  int16_t* coef = coef_all + a.page_base[4 * pg];
  const DcScan sc = sync_dc_scan(d, c);
  const uint32_t L = sc.L, seg = sc.seg;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < L; base += 2048) {
    uint32_t loc[8], run = 0, flag = 0;
    int first_reset = 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t e = base + tid * 8 + j;
      if (e < L) {
        if (e % seg == 0) { run = 0; if (!flag) { flag = 1; first_reset = j; } }
        run += (uint32_t)(int32_t)coef[sync_dc_addr(d, c, e)];
      }
      loc[j] = run;
    }
    s_v[tid] = run; s_f[tid] = flag;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {       // inclusive scan of (flag, value): a flag cuts what comes from the left
      uint32_t v = s_v[tid], fl = s_f[tid];
      if (tid >= off) { if (!fl) v += s_v[tid - off]; fl |= s_f[tid - off]; }
      __syncthreads();
      s_v[tid] = v; s_f[tid] = fl;
      __syncthreads();
    }
    const uint32_t left = tid ? (s_f[tid - 1] ? s_v[tid - 1] : s_v[tid - 1] + carry) : carry;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t e = base + tid * 8 + j;
      if (e < L) coef[sync_dc_addr(d, c, e)] = (int16_t)(loc[j] + (j < first_reset ? left : 0u));
    }
    const uint32_t next = s_f[255] ? s_v[255] : s_v[255] + carry;
    __syncthreads();
    carry = next;
  }
}

// ---------------------------------------------------------------------------------------------------- reconstruction
// jidctint.c, jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2
#define C_0_298631336 2446
#define C_0_390180644 3196
#define C_0_541196100 4433
#define C_0_765366865 6270
#define C_0_899976223 7373
#define C_1_175875602 9633
#define C_1_501321110 12299
#define C_1_847759065 15137
#define C_1_961570560 16069
#define C_2_053119869 16819
#define C_2_562915447 20995
#define C_3_072711026 25172

// All IDCT arithmetic is done modulo 2^32 on unsigned words (identical to libjpeg's signed arithmetic wherever that does not
// overflow, i.e. for every stream an encoder can produce; a hostile stream wraps instead of being undefined behaviour).
typedef uint32_t U32;
HD int descale(U32 x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }
HD uint8_t idct_range_limit(int v) {  // sample_range_limit + CENTERJSAMPLE, indexed with (v & RANGE_MASK)
  const int x = v & 1023;
  return (uint8_t)(x < 128 ? x + 128 : (x < 512 ? 255 : (x < 896 ? 0 : x - 896)));
}

HD void idct_1d(U32 d0, U32 d1, U32 d2, U32 d3, U32 d4, U32 d5, U32 d6, U32 d7, int shift0, int o[8]) {
  // even part; d0/d4 are shifted up by CONST_BITS by the caller's convention: tmp0 = (d0 + d4) << CONST_BITS
  U32 z1 = (d2 + d6) * (U32)C_0_541196100;
  const U32 t2 = z1 + d6 * (U32)(-C_1_847759065);
  const U32 t3 = z1 + d2 * (U32)C_0_765366865;
  const U32 t0 = (d0 + d4) << 13;
  const U32 t1 = (d0 - d4) << 13;
  const U32 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  // odd part
  U32 a0 = d7, a1 = d5, a2 = d3, a3 = d1;
  z1 = a0 + a3;
  U32 z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const U32 z5 = (z3 + z4) * (U32)C_1_175875602;
  a0 *= (U32)C_0_298631336; a1 *= (U32)C_2_053119869; a2 *= (U32)C_3_072711026; a3 *= (U32)C_1_501321110;
  z1 *= (U32)(-C_0_899976223); z2 *= (U32)(-C_2_562915447); z3 *= (U32)(-C_1_961570560); z4 *= (U32)(-C_0_390180644);
  z3 += z5; z4 += z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  o[0] = descale(t10 + a3, shift0); o[7] = descale(t10 - a3, shift0);
  o[1] = descale(t11 + a2, shift0); o[6] = descale(t11 - a2, shift0);
  o[2] = descale(t12 + a1, shift0); o[5] = descale(t12 - a1, shift0);
  o[3] = descale(t13 + a0, shift0); o[4] = descale(t13 - a0, shift0);
}

// one 8x8 block: coefficients (natural order) x quantisation table -> 64 samples, row-major with `ld` bytes between rows
HD void idct_block(const int16_t* coef, const uint16_t* q, uint8_t* out, long ld) {
  int ws[64];
  auto dq = [&](int k) { return (U32)(int32_t)coef[k] * (U32)q[k]; };
  for (int c = 0; c < 8; ++c) {  // pass 1: columns (the all-AC-zero shortcut of the reference gives the same values)
    int o[8];
    idct_1d(dq(c), dq(8 + c), dq(16 + c), dq(24 + c), dq(32 + c), dq(40 + c), dq(48 + c), dq(56 + c), 13 - 2, o);
    for (int r = 0; r < 8; ++r) ws[r * 8 + c] = o[r];
  }
  for (int r = 0; r < 8; ++r) {  // pass 2: rows
    int o[8];
    const int* w = ws + r * 8;
    idct_1d((U32)w[0], (U32)w[1], (U32)w[2], (U32)w[3], (U32)w[4], (U32)w[5], (U32)w[6], (U32)w[7], 13 + 2 + 3, o);
    for (int c = 0; c < 8; ++c) out[r * ld + c] = idct_range_limit(o[c]);
  }
}

struct Planes {
  uint8_t* p[3];
  int ld[3];       // bytes per plane row (blocks_w * 8)
  int dsw[3], dsh[3];  // real (unpadded) extent of the component: ceil(image * samp / max)
};

// chroma sample at full-resolution position (X, Y): jdsample.c fullsize / h2v1 / h2v2, fancy (triangle) filters when the
// downsampled width is > 2, plain replication otherwise
HD int chroma_at(const uint8_t* pl, int ld, int dsw, int dsh, int hfac, int vfac, int X, int Y) {
  if (hfac == 1 && vfac == 1) return pl[(long)Y * ld + X];
  const int c = X >> 1;
  if (vfac == 1) {  // h2v1
    const uint8_t* row = pl + (long)Y * ld;
    if (dsw <= 2) return row[c];
    if (!(X & 1)) return c == 0 ? row[0] : (row[c] * 3 + row[c - 1] + 1) >> 2;
    return c == dsw - 1 ? row[c] : (row[c] * 3 + row[c + 1] + 2) >> 2;
  }
  const int r = Y >> 1;  // h2v2
  if (dsw <= 2) return pl[(long)r * ld + c];
  int rn = (Y & 1) ? r + 1 : r - 1;  // nearer neighbour row; the first / last real row is its own neighbour at the image edge
  rn = rn < 0 ? 0 : (rn > dsh - 1 ? dsh - 1 : rn);
  const uint8_t* r0 = pl + (long)r * ld;
  const uint8_t* r1 = pl + (long)rn * ld;
  const int cur = r0[c] * 3 + r1[c];
  if (!(X & 1)) {
    if (c == 0) return (cur * 4 + 8) >> 4;
    return (cur * 3 + (r0[c - 1] * 3 + r1[c - 1]) + 8) >> 4;
  }
  if (c == dsw - 1) return (cur * 4 + 7) >> 4;
  return (cur * 3 + (r0[c + 1] * 3 + r1[c + 1]) + 7) >> 4;
}

HD uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// jdcolor.c ycc_rgb_convert: SCALEBITS 16 tables, evaluated directly
HD void ycc_to_rgb(int y, int cb, int cr, uint8_t* o) {
  const int xb = cb - 128, xr = cr - 128;
  const int cr_r = (91881 * xr + 32768) >> 16;
  const int cb_b = (116130 * xb + 32768) >> 16;
  const int g = (-22554 * xb + 32768 + (-46802) * xr) >> 16;
  o[0] = clamp255(y + cr_r);
  o[1] = clamp255(y + g);
  o[2] = clamp255(y + cb_b);
}

HD void pixel_rgb(const msocr_jpeg_info& f, const Planes& pl, int X, int Y, uint8_t* o) {
  const int y = pl.p[0][(long)Y * pl.ld[0] + X];
  if (f.ncomp == 1) {
    o[0] = o[1] = o[2] = (uint8_t)y;
    return;
  }
  const int cb = chroma_at(pl.p[1], pl.ld[1], pl.dsw[1], pl.dsh[1], f.hs[0], f.vs[0], X, Y);
  const int cr = chroma_at(pl.p[2], pl.ld[2], pl.dsw[2], pl.dsh[2], f.hs[0], f.vs[0], X, Y);
  ycc_to_rgb(y, cb, cr, o);
}

Planes make_planes(const msocr_jpeg_info& f, uint8_t* base) {
  Planes pl;
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    pl.p[c] = nullptr; pl.ld[c] = 0; pl.dsw[c] = 0; pl.dsh[c] = 0;
    if (c < f.ncomp) {
      pl.p[c] = base + off;
      pl.ld[c] = f.blocks_w[c] * 8;
      pl.dsw[c] = (f.width * f.hs[c] + f.hs[0] - 1) / f.hs[0];
      pl.dsh[c] = (f.height * f.vs[c] + f.vs[0] - 1) / f.vs[0];
      off += ((int64_t)f.blocks_w[c] * f.blocks_h[c] * 64 + 255) / 256 * 256;
    }
  }
  return pl;
}

int64_t planes_bytes(const msocr_jpeg_info& f) {
  int64_t off = 0;
  for (int c = 0; c < f.ncomp; ++c) off += ((int64_t)f.blocks_w[c] * f.blocks_h[c] * 64 + 255) / 256 * 256;
  return off;
}

bool info_ok(const msocr_jpeg_info* f) {
  if (!f || f->supported != 1 || (f->ncomp != 1 && f->ncomp != 3) || f->width <= 0 || f->height <= 0) return false;
  // the sampling forms a parse produces, the only ones chroma_at knows: 1x1 (grey, 4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) for the
  // first component, 1x1 for the others
  if (!((f->hs[0] == 1 && f->vs[0] == 1) || (f->hs[0] == 2 && f->vs[0] == 1) || (f->hs[0] == 2 && f->vs[0] == 2))) return false;
  int64_t off = 0;
  for (int c = 0; c < f->ncomp; ++c) {
    if (c > 0 && (f->hs[c] != 1 || f->vs[c] != 1)) return false;
    if (f->blocks_w[c] <= 0 || f->blocks_h[c] <= 0) return false;
    if (f->coef_off[c] != off) return false;
    if ((int64_t)f->blocks_w[c] * 8 * f->hs[0] / f->hs[c] < f->width || (int64_t)f->blocks_h[c] * 8 * f->vs[0] / f->vs[c] < f->height) return false;
    off += (int64_t)f->blocks_w[c] * f->blocks_h[c] * 64;
  }
  return off == f->coef_total;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(msocr_jpeg_info f, const int16_t* __restrict__ coef, Planes pl) {
  const long nb0 = (long)f.blocks_w[0] * f.blocks_h[0];
  const long nb1 = f.ncomp == 3 ? (long)f.blocks_w[1] * f.blocks_h[1] : 0;
  const long total = nb0 + 2 * nb1;
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < total; b += (long)gridDim.x * 256) {
    int c = 0;
    long k = b;
    if (k >= nb0) { k -= nb0; c = 1; if (k >= nb1) { k -= nb1; c = 2; } }
    const int by = (int)(k / f.blocks_w[c]), bx = (int)(k - (long)by * f.blocks_w[c]);
    idct_block(coef + f.coef_off[c] + k * 64, f.quant[c], pl.p[c] + ((long)by * 8) * pl.ld[c] + bx * 8, pl.ld[c]);
  }
}

// ---------------------------------------------------------------------------------------------------- Exif orientation
// Where source pixel (X, Y) of a W x H frame goes under Exif orientation 2..8 (what ImageOps.exif_transpose / cv2.imread do);
// the output is [H][W][3] for 2..4 and [W][H][3] for 5..8.  Kernels and host twin share it.
HD bool orient_transposes(int o) { return o >= 5; }
HD bool orient_flips_x(int o) { return o == 2 || o == 3 || o == 7 || o == 8; }   // the X term is W-1-X
HD bool orient_flips_y(int o) { return o == 3 || o == 4 || o == 6 || o == 7; }   // the Y term is H-1-Y
HD int64_t orient_dest(int o, int W, int H, int X, int Y) {
  const int x = orient_flips_x(o) ? W - 1 - X : X, y = orient_flips_y(o) ? H - 1 - Y : Y;
  return orient_transposes(o) ? (int64_t)x * H + y : (int64_t)y * W + x;
}

// The colour stage in source-row order, orientations 1..4.  MIRRORED = false: upright, pixel i goes to place i and there is no
// remap code; true (2..4): the destination is remapped.  Rows stay rows either way: a wave's stores cover one contiguous run of
// a destination row (descending where X is mirrored).
template <bool MIRRORED>
__global__ __launch_bounds__(256) void jpeg_color_kernel(msocr_jpeg_info f, Planes pl, int o, uint8_t* __restrict__ rgb) {
  const long total = (long)f.width * f.height;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int Y = (int)(i / f.width), X = (int)(i - (long)Y * f.width);
    uint8_t px[3];
    pixel_rgb(f, pl, X, Y, px);
    const int64_t d = 3 * (MIRRORED ? orient_dest(o, f.width, f.height, X, Y) : (int64_t)i);
    rgb[d] = px[0]; rgb[d + 1] = px[1]; rgb[d + 2] = px[2];
  }
}

// Orientations 5..8: a source row becomes a destination column.  One workgroup per kOrientTile x kOrientTile tile of source pixels
// (grid = tiles in X, tiles in Y): pixel_rgb in source-row order (a wave = 64 consecutive X of one row, the plane reads of
// jpeg_color_kernel), the packed pixel parked in LDS as one dword at [sy][sx]; after the barrier every wave writes destination
// rows of the tile (one per sx: the tile's ny pixels at consecutive columns), lane p the three bytes of pixel p as
// jpeg_color_kernel stores them: the wave's three byte stores cover one contiguous run of 3 * ny bytes.  LDS pitch
// kOrientTile + 1 dwords: the read-back walks sy at one sx, bank (sy * 65 + sx) mod 32 = (sy + sx) mod 32, all different within
// a 32-lane half; the writes walk sx: consecutive banks.  Measured against one byte per lane on consecutive bytes (48 stores per
// thread, an LDS read and a division by 3 each): 0.71 against 0.85 ms per 16 pages.
constexpr int kOrientTile = 64;
constexpr int kOrientPitch = kOrientTile + 1;
__global__ __launch_bounds__(256) void jpeg_color_transpose_kernel(msocr_jpeg_info f, Planes pl, int o, uint8_t* __restrict__ rgb) {
  __shared__ uint32_t tile[kOrientTile * kOrientPitch];
  const int W = f.width, H = f.height;
  const int X0 = blockIdx.x * kOrientTile, Y0 = blockIdx.y * kOrientTile;
  const int nx = W - X0 < kOrientTile ? W - X0 : kOrientTile, ny = H - Y0 < kOrientTile ? H - Y0 : kOrientTile;
  const int lane = threadIdx.x & (kOrientTile - 1), first = threadIdx.x / kOrientTile;
  constexpr int kStep = 256 / kOrientTile;
  if (lane < nx) {
    for (int sy = first; sy < ny; sy += kStep) {
      uint8_t px[3];
      pixel_rgb(f, pl, X0 + lane, Y0 + sy, px);
      tile[sy * kOrientPitch + lane] = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
    }
  }
  __syncthreads();
  if (lane < ny) {
    const int sy = orient_flips_y(o) ? ny - 1 - lane : lane;   // the wave's addresses ascend with the lane either way
    for (int sx = first; sx < nx; sx += kStep) {
      const uint32_t v = tile[sy * kOrientPitch + sx];
      const int64_t d = 3 * orient_dest(o, W, H, X0 + sx, Y0 + sy);
      rgb[d] = (uint8_t)v; rgb[d + 1] = (uint8_t)(v >> 8); rgb[d + 2] = (uint8_t)(v >> 16);
    }
  }
}

// blocks of 256 threads for a grid-stride loop over n elements
unsigned stride_grid(long n) {
  const long g = (n + 255) / 256;
  return (unsigned)(g > 65535 ? 65535 : g);
}

// The device reconstruction behind both entries: IDCT into the planes of the workspace, then the colour stage whose last write
// applies the orientation: 1 = upright, 2..4 = mirrored destinations, 5..8 = the tiled transposing kernel.
int reconstruct(const msocr_jpeg_info* info, int orientation, const int16_t* coef_dev, void* workspace_dev, uint8_t* rgb_out_dev,
                hipStream_t s) {
  if (orientation < 1 || orientation > 8 || !info_ok(info) || !coef_dev || !workspace_dev || !rgb_out_dev || ((uintptr_t)workspace_dev & 15))
    return MSOCR_E_ARG;
  const Planes pl = make_planes(*info, (uint8_t*)workspace_dev);
  MSOCR_LAUNCH(jpeg_idct_kernel, dim3(stride_grid((long)info->coef_total / 64)), dim3(256), 0, s, *info, coef_dev, pl);
  if (hipGetLastError() != hipSuccess) return MSOCR_E_LAUNCH;
  const dim3 rows(stride_grid((long)info->width * info->height));
  if (orient_transposes(orientation)) {
    const dim3 grid((unsigned)((info->width + kOrientTile - 1) / kOrientTile), (unsigned)((info->height + kOrientTile - 1) / kOrientTile));
    MSOCR_LAUNCH(jpeg_color_transpose_kernel, grid, dim3(256), 0, s, *info, pl, orientation, rgb_out_dev);
  } else if (orientation == 1) {
    MSOCR_LAUNCH(jpeg_color_kernel<false>, rows, dim3(256), 0, s, *info, pl, orientation, rgb_out_dev);
  } else {
    MSOCR_LAUNCH(jpeg_color_kernel<true>, rows, dim3(256), 0, s, *info, pl, orientation, rgb_out_dev);
  }
  return hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH;
}

void idct_planes_host(const msocr_jpeg_info* info, const int16_t* coef_host, const Planes& pl) {
  for (int c = 0; c < info->ncomp; ++c)
    for (int by = 0; by < info->blocks_h[c]; ++by)
      for (int bx = 0; bx < info->blocks_w[c]; ++bx)
        idct_block(coef_host + info->coef_off[c] + ((int64_t)by * info->blocks_w[c] + bx) * 64, info->quant[c],
                   pl.p[c] + ((long)by * 8) * pl.ld[c] + bx * 8, pl.ld[c]);
}

// The host twin behind both entries: the same idct_block, pixel_rgb and orient_dest (orientation 1: no flips, no transpose).
int reconstruct_host(const msocr_jpeg_info* info, int orientation, const int16_t* coef_host, uint8_t* rgb_out_host) {
  if (orientation < 1 || orientation > 8 || !info_ok(info) || !coef_host || !rgb_out_host) return MSOCR_E_ARG;
  std::vector<uint8_t> ws((size_t)planes_bytes(*info));
  const Planes pl = make_planes(*info, ws.data());
  idct_planes_host(info, coef_host, pl);
  for (int Y = 0; Y < info->height; ++Y)
    for (int X = 0; X < info->width; ++X)
      pixel_rgb(*info, pl, X, Y, rgb_out_host + 3 * orient_dest(orientation, info->width, info->height, X, Y));
  return MSOCR_OK;
}

}  // namespace

extern "C" int msocr_jpeg_parse_host(const uint8_t* data_host, int64_t len, msocr_jpeg_info* info_out) {
  if (!info_out) return MSOCR_E_ARG;
  Parsed P;
  const int rc = parse(data_host, len, &P);
  *info_out = P.info;
  if (rc != MSOCR_OK) info_out->supported = 0;
  return rc;
}

extern "C" int msocr_jpeg_parse_oriented_host(const uint8_t* data_host, int64_t len, msocr_jpeg_info* info_out, int32_t* orientation_out) {
  if (!info_out || !orientation_out) return MSOCR_E_ARG;
  Parsed P;
  const int rc = parse(data_host, len, &P, kExifReport, orientation_out);
  *info_out = P.info;
  if (rc != MSOCR_OK) { info_out->supported = 0; *orientation_out = 1; }
  return rc;
}

extern "C" int msocr_jpeg_entropy_decode_host(const uint8_t* data_host, int64_t len, const msocr_jpeg_info* info, int16_t* coef_out_host) {
  Parsed P;
  if (!coef_out_host || reparse(data_host, len, info, &P) != MSOCR_OK) return MSOCR_E_ARG;
  return entropy_decode(P, data_host + len, coef_out_host);
}

extern "C" int64_t msocr_jpeg_scan_desc_bytes(void) { return (int64_t)sizeof(ScanDesc); }

// Walks the entropy-coded segment with entropy_decode's own interval_walk: interval k ends at the first marker (0xFF not followed
// by 0x00) at or after its start, interval k + 1 starts behind the first RSTn at or after that marker.
// `serial_too`: a stream without DRI is taken as ONE interval of all its MCUs (the self-synchronising stage's view of it)
static int64_t scan_prepare(const uint8_t* data_host, int64_t len, const msocr_jpeg_info* info, int64_t bytes_base, void* desc_out,
                            uint32_t* bounds_out, int64_t bounds_cap, bool serial_too) {
  Parsed P;
  if (!data_host || !desc_out || !bounds_out || bytes_base < 0 || reparse(data_host, len, info, &P) != MSOCR_OK) return MSOCR_E_ARG;
  const int64_t total = (int64_t)P.mcus_x * P.mcus_y;
  if (P.restart_interval <= 0) {
    if (!serial_too || total > 0x7fffffff) return MSOCR_E_ARG;           // one serial bit stream: not the per-interval kernel's
    P.restart_interval = (int)total;
  }
  // interval bounds are 32-bit offsets into the file; the self-synchronising stage keeps BIT positions in 32 bits
  if (len > (serial_too ? 0x1ff00000LL : 0xfffffff0LL)) return MSOCR_E_ARG;
  const int64_t n_iv = (total + P.restart_interval - 1) / P.restart_interval;
  if (n_iv > bounds_cap || n_iv > 0x7fffffff) return MSOCR_E_ARG;
  ScanDesc* d = static_cast<ScanDesc*>(desc_out);
  memset(d, 0, sizeof(*d));
  d->info = P.info;
  d->bytes_base = bytes_base;
  d->restart_interval = P.restart_interval;
  d->mcus_x = P.mcus_x; d->mcus_y = P.mcus_y; d->n_intervals = (int32_t)n_iv;
  for (int c = 0; c < P.info.ncomp; ++c) {
    d->dc[c] = P.dc[P.dc_sel[c]].lut;
    d->ac[c] = P.ac[P.ac_sel[c]].lut;
  }
  memcpy(d->zigzag, kZigzag, 64);
  const uint8_t* const end = data_host + len;
  const uint8_t* p = P.scan;
  for (int64_t k = 0; k < n_iv; ++k) {
    const uint8_t* e;
    const uint8_t* const next = interval_walk(p, end, &e);
    bounds_out[2 * k] = (uint32_t)(p - data_host);
    bounds_out[2 * k + 1] = (uint32_t)(e - data_host);
    if (k + 1 < n_iv && !next) return MSOCR_E_ARG;
    p = next;
  }
  return n_iv;
}

extern "C" int64_t msocr_jpeg_scan_prepare_host(const uint8_t* data_host, int64_t len, const msocr_jpeg_info* info, int64_t bytes_base,
                                                void* desc_out, uint32_t* bounds_out, int64_t bounds_cap) {
  return scan_prepare(data_host, len, info, bytes_base, desc_out, bounds_out, bounds_cap, false);
}

extern "C" int64_t msocr_jpeg_sync_prepare_host(const uint8_t* data_host, int64_t len, const msocr_jpeg_info* info, int64_t bytes_base,
                                                void* desc_out, uint32_t* bounds_out, int64_t bounds_cap) {
  return scan_prepare(data_host, len, info, bytes_base, desc_out, bounds_out, bounds_cap, true);
}

extern "C" int msocr_jpeg_entropy_decode_device(const uint8_t* bytes_dev, const void* descs_dev, int32_t n_pages, int32_t max_intervals,
                                                const uint32_t* bounds_dev, const int64_t* page_base_dev, int16_t* coef_dev,
                                                int64_t coef_total, int32_t* status_dev, void* stream) {
  if (!bytes_dev || !descs_dev || !bounds_dev || !page_base_dev || !coef_dev || !status_dev || n_pages <= 0 || n_pages > 65535 ||
      max_intervals <= 0 || coef_total <= 0 || (((uintptr_t)descs_dev | (uintptr_t)page_base_dev) & 7))
    return MSOCR_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(coef_dev, 0, (size_t)coef_total * sizeof(int16_t), s) != hipSuccess) return MSOCR_E_LAUNCH;
  if (hipMemsetAsync(status_dev, 0, (size_t)n_pages * sizeof(int32_t), s) != hipSuccess) return MSOCR_E_LAUNCH;
  // wave slots wanted: two per SIMD of the device; lanes per wave = the power of two that fills them
  int n_cu = 0;
  if (msocr_internal_cu_count(&n_cu) != MSOCR_OK) return MSOCR_E_LAUNCH;
  const int slots = n_cu * 8;
  int lanes = 1;
  while (lanes < 64 && (int64_t)n_pages * max_intervals > (int64_t)slots * lanes) lanes *= 2;
  MSOCR_LAUNCH(jpeg_huffman_kernel, dim3((unsigned)((max_intervals + lanes - 1) / lanes), (unsigned)n_pages), dim3(64), 0, s, bytes_dev,
               static_cast<const ScanDesc*>(descs_dev), bounds_dev, page_base_dev, coef_dev, status_dev, lanes);
  return hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH;
}

// HOST twin of jpeg_huffman_kernel: the same decode_interval, interval after interval (all pointers host memory).
extern "C" int msocr_jpeg_entropy_decode_intervals_host(const uint8_t* bytes_host, const void* descs_host, int32_t n_pages,
                                                        const uint32_t* bounds_host, const int64_t* page_base_host, int16_t* coef_host,
                                                        int64_t coef_total, int32_t* status_host) {
  if (!bytes_host || !descs_host || !bounds_host || !page_base_host || !coef_host || !status_host || n_pages <= 0 || coef_total <= 0)
    return MSOCR_E_ARG;
  memset(coef_host, 0, (size_t)coef_total * sizeof(int16_t));
  const ScanDesc* descs = static_cast<const ScanDesc*>(descs_host);
  for (int pg = 0; pg < n_pages; ++pg) {
    const ScanDesc& d = descs[pg];
    status_host[pg] = 0;
    const int64_t coef_base = page_base_host[2 * pg], first_interval = page_base_host[2 * pg + 1];
    if (coef_base < 0 || coef_base + d.info.coef_total > coef_total || first_interval < 0) return MSOCR_E_ARG;
    for (int iv = 0; iv < d.n_intervals; ++iv) {
      const int first = iv * d.restart_interval;
      if (decode_interval(d.info, d.mcus_x, d.dc, d.ac, d.zigzag, bytes_host + d.bytes_base, bounds_host[2 * (first_interval + iv)],
                          bounds_host[2 * (first_interval + iv) + 1], first, interval_mcus(d.mcus_x * d.mcus_y, d.restart_interval, first),
                          coef_host + coef_base))
        status_host[pg] = 1;
    }
  }
  return MSOCR_OK;
}

extern "C" int64_t msocr_jpeg_sync_workspace_bytes(int64_t total_subseq, int32_t n_pages, int32_t max_rounds) {
  if (total_subseq <= 0 || n_pages <= 0 || max_rounds < 2 || max_rounds > 65536) return -1;
  int64_t off[6];
  return sync_layout(total_subseq, n_pages, max_rounds, off);
}

static bool sync_args_ok(const void* bytes, const void* descs, int32_t n_pages, const void* bounds, const void* sub_first,
                         const void* page_base, int64_t total_subseq, int32_t subseq_bytes, int32_t max_rounds, const void* coef,
                         int64_t coef_total, const void* status, const void* workspace) {
  return bytes && descs && bounds && sub_first && page_base && coef && status && workspace && n_pages > 0 && n_pages <= 65535 &&
         total_subseq > 0 && subseq_bytes >= 16 && subseq_bytes <= 65536 && max_rounds >= 2 && max_rounds <= 65536 && coef_total > 0 &&
         !(((uintptr_t)descs | (uintptr_t)page_base | (uintptr_t)workspace) & 7);
}

extern "C" int msocr_jpeg_entropy_decode_sync_device(const uint8_t* bytes_dev, const void* descs_dev, int32_t n_pages,
                                                     const uint32_t* bounds_dev, const uint32_t* sub_first_dev,
                                                     const int64_t* page_base_dev, int32_t max_subseq, int64_t total_subseq,
                                                     int32_t subseq_bytes, int32_t max_rounds, int16_t* coef_dev, int64_t coef_total,
                                                     int32_t* status_dev, int32_t* rounds_dev, void* workspace_dev, void* stream) {
  if (!sync_args_ok(bytes_dev, descs_dev, n_pages, bounds_dev, sub_first_dev, page_base_dev, total_subseq, subseq_bytes, max_rounds,
                    coef_dev, coef_total, status_dev, workspace_dev) || max_subseq <= 0 || max_subseq > total_subseq)
    return MSOCR_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  SyncArgs a;
  a.bytes = bytes_dev; a.descs = static_cast<const ScanDesc*>(descs_dev); a.bounds = bounds_dev; a.sub_first = sub_first_dev;
  a.page_base = page_base_dev; a.S = (uint32_t)subseq_bytes; a.n_pages = n_pages; a.max_rounds = max_rounds;
  a.w = sync_workspace(workspace_dev, total_subseq, n_pages, max_rounds);
  if (hipMemsetAsync(coef_dev, 0, (size_t)coef_total * sizeof(int16_t), s) != hipSuccess) return MSOCR_E_LAUNCH;
  if (hipMemsetAsync(status_dev, 0, (size_t)n_pages * sizeof(int32_t), s) != hipSuccess) return MSOCR_E_LAUNCH;
  if (hipMemsetAsync(a.w.changed, 0, (size_t)max_rounds * n_pages * sizeof(int32_t), s) != hipSuccess) return MSOCR_E_LAUNCH;
  const dim3 grid((unsigned)((max_subseq + 255) / 256), (unsigned)n_pages);
  // a fixed number of rounds, nobody waits in between: the kernels of a page that stands return at once
  for (int r = 0; r < max_rounds; ++r) MSOCR_LAUNCH(jpeg_sync_round_kernel, grid, dim3(256), 0, s, a, r);
  MSOCR_LAUNCH(jpeg_sync_place_kernel, dim3((unsigned)n_pages), dim3(256), 0, s, a, status_dev, rounds_dev);
  MSOCR_LAUNCH(jpeg_sync_write_kernel, grid, dim3(256), 0, s, a, coef_dev, status_dev);
  MSOCR_LAUNCH(jpeg_sync_dc_kernel, dim3(3, (unsigned)n_pages), dim3(256), 0, s, a, coef_dev);
  return hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH;
}

// HOST twin of the kernel sequence: the same rounds (double-buffered exit states, a page stops when a round changed nothing), the
// same prefix sums, write pass and DC sums, subsequence after subsequence (all pointers host memory; no workspace).
extern "C" int msocr_jpeg_entropy_decode_sync_host(const uint8_t* bytes_host, const void* descs_host, int32_t n_pages,
                                                   const uint32_t* bounds_host, const uint32_t* sub_first_host,
                                                   const int64_t* page_base_host, int32_t subseq_bytes, int32_t max_rounds,
                                                   int16_t* coef_host, int64_t coef_total, int32_t* status_host, int32_t* rounds_host) {
  int64_t dummy[1];
  if (!sync_args_ok(bytes_host, descs_host, n_pages, bounds_host, sub_first_host, page_base_host, 1, subseq_bytes, max_rounds, coef_host,
                    coef_total, status_host, dummy))
    return MSOCR_E_ARG;
  memset(coef_host, 0, (size_t)coef_total * sizeof(int16_t));
  const ScanDesc* descs = static_cast<const ScanDesc*>(descs_host);
  const uint32_t S = (uint32_t)subseq_bytes;
  for (int pg = 0; pg < n_pages; ++pg) {
    const ScanDesc& d = descs[pg];
    const int64_t* pb = page_base_host + 4 * pg;
    status_host[pg] = 0;
    if (pb[0] < 0 || pb[0] + d.info.coef_total > coef_total || pb[1] < 0 || pb[3] <= 0 || pb[3] > 0x7fffffff || d.n_intervals <= 0)
      return MSOCR_E_ARG;
    const uint32_t nsub = (uint32_t)pb[3];
    const uint8_t* bytes = bytes_host + d.bytes_base;
    const uint32_t *bounds = bounds_host + 2 * pb[1], *sub_first = sub_first_host + pb[1];
    std::vector<uint64_t> entry(nsub), ex0(nsub), ex1(nsub);
    std::vector<uint32_t> cnt(nsub), P((size_t)nsub + 1);
    std::vector<int32_t> changed((size_t)max_rounds, 0);
    uint64_t* ex[2] = {ex0.data(), ex1.data()};
    for (int r = 0; r < max_rounds; ++r) {
      if (r >= 2 && !changed[r - 1]) break;
      for (uint32_t i = 0; i < nsub; ++i)
        if (sync_round(d, d.dc, d.ac, d.zigzag, bytes, bounds, sub_first, nsub, S, i, r, entry.data(), ex[(r + 1) & 1], ex[r & 1], cnt.data()) &&
            r >= 1)
          changed[r] = 1;
    }
    int declined;
    const int rounds = sync_rounds_taken(changed.data(), 1, max_rounds, nsub, &declined);
    if (rounds_host) rounds_host[pg] = rounds;
    if (declined) { status_host[pg] = 2; continue; }
    P[0] = 0;
    for (uint32_t i = 0; i < nsub; ++i) P[i + 1] = P[i] + cnt[i];
    int16_t* coef = coef_host + pb[0];
    for (uint32_t i = 0; i < nsub; ++i) {
      const int st = sync_write(d, d.dc, d.ac, d.zigzag, bytes, bounds, sub_first, nsub, S, i, entry.data(), P.data(), coef);
      if (st > status_host[pg]) status_host[pg] = st;
    }
    for (int c = 0; c < d.info.ncomp; ++c) {
      const DcScan sc = sync_dc_scan(d, c);
      uint32_t run = 0;
      for (uint32_t e = 0; e < sc.L; ++e) {
        if (e % sc.seg == 0) run = 0;
        const int64_t at = sync_dc_addr(d, c, e);
        run += (uint32_t)(int32_t)coef[at];
        coef[at] = (int16_t)run;
      }
    }
  }
  return MSOCR_OK;
}

extern "C" int64_t msocr_jpeg_workspace_bytes(const msocr_jpeg_info* info) { return info_ok(info) ? planes_bytes(*info) : -1; }

extern "C" int msocr_jpeg_reconstruct(const msocr_jpeg_info* info, const int16_t* coef_dev, void* workspace_dev, uint8_t* rgb_out_dev,
                                      void* stream) {
  return reconstruct(info, 1, coef_dev, workspace_dev, rgb_out_dev, (hipStream_t)stream);
}

extern "C" int msocr_jpeg_reconstruct_host(const msocr_jpeg_info* info, const int16_t* coef_host, uint8_t* rgb_out_host) {
  return reconstruct_host(info, 1, coef_host, rgb_out_host);
}

// The reconstruction with the Exif orientation applied in its last write; 1 = msocr_jpeg_reconstruct.  The IDCT stage and the
// workspace are the same for every orientation.
extern "C" int msocr_jpeg_reconstruct_oriented(const msocr_jpeg_info* info, int32_t orientation, const int16_t* coef_dev,
                                               void* workspace_dev, uint8_t* rgb_out_dev, void* stream) {
  return reconstruct(info, orientation, coef_dev, workspace_dev, rgb_out_dev, (hipStream_t)stream);
}

extern "C" int msocr_jpeg_reconstruct_oriented_host(const msocr_jpeg_info* info, int32_t orientation, const int16_t* coef_host,
                                                    uint8_t* rgb_out_host) {
  return reconstruct_host(info, orientation, coef_host, rgb_out_host);
}
