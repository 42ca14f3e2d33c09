// The marker walk of the baseline JPEG decoder: everything in front of the scan of a file as PIL.Image.save and
// cv2.imwrite write it by default (baseline SOF0, 8 bit, 4:2:0 or one component, one scan, no restart interval, JFIF),
// into a plain irx_jpeg_info; every other kind of file is refused with a status of its own (include/irx.h) and stays
// with PIL.  The tables are read from the file, never assumed to be Annex K.  Host only, plain C++ (no HIP);
// jpeg_host.parse is the same walk in Python.
#include <cstring>
#include <exception>
#include <string>

#include "../../include/irx.h"
#include "jpeg_tables.h"

namespace irx {
void set_error(const std::string& msg);   // capi.cpp
}

namespace {

using irx::jpegtab::kZigzag;

int fail(int status, const std::string& msg) {
  irx::set_error("irx_jpeg_parse: " + msg);
  return status;
}

constexpr int kMinSide = 8;   // the inverse half's minimum (irx_degrade_jpeg refuses less)

int parse(const uint8_t* d, long n, irx_jpeg_info* info) {
  std::memset(info, 0, sizeof(*info));
  if (n == 0) return fail(IRX_JPEG_NOT_JPEG, "empty file");
  if (n < 2) return fail(IRX_JPEG_TRUNCATED, "truncated file");
  if (d[0] != 0xFF || d[1] != 0xD8) return fail(IRX_JPEG_NOT_JPEG, "no SOI marker");
  bool have_sof = false;
  int comp_id[3] = {0, 0, 0};
  long p = 2;
  for (;;) {
    if (p + 4 > n) return fail(IRX_JPEG_TRUNCATED, "file ends in the header");
    if (d[p] != 0xFF) return fail(IRX_JPEG_MALFORMED, "marker expected");
    const int m = d[p + 1];
    if (m == 0xFF) {                                         // fill byte
      ++p;
      continue;
    }
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7))
      return fail(IRX_JPEG_MALFORMED, "stand-alone marker in the header");
    if (m == 0xD9) return fail(IRX_JPEG_MALFORMED, "EOI before a scan");
    const long ln = ((long)d[p + 2] << 8) | d[p + 3];
    if (ln < 2) return fail(IRX_JPEG_MALFORMED, "segment length below 2");
    if (p + 2 + ln > n) return fail(IRX_JPEG_TRUNCATED, "file ends in a segment");
    const uint8_t* seg = d + p + 4;                          // the segment's payload: seg[0 .. sl)
    const long sl = ln - 2;
    p += 2 + ln;
    if (m == 0xC0) {
      if (have_sof) return fail(IRX_JPEG_MALFORMED, "two frame headers");
      if (sl < 6) return fail(IRX_JPEG_MALFORMED, "short SOF0");
      if (seg[0] != 8) return fail(IRX_JPEG_PRECISION, "sample precision other than 8 bits");
      const int H = (seg[1] << 8) | seg[2], W = (seg[3] << 8) | seg[4], nc = seg[5];
      if (nc == 4) return fail(IRX_JPEG_COMPONENTS, "four components (CMYK / YCCK)");
      if (nc != 1 && nc != 3) return fail(IRX_JPEG_COMPONENTS, "1 or 3 components");
      if (sl != 6 + 3 * nc) return fail(IRX_JPEG_MALFORMED, "SOF0 length");
      for (int i = 0; i < nc; ++i) {
        comp_id[i] = seg[6 + 3 * i];
        info->qsel[i] = seg[8 + 3 * i];
      }
      if (nc == 3) {
        if (comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
          return fail(IRX_JPEG_RGB_IDS, "component ids R, G, B");
        if (seg[7] != 0x22 || seg[10] != 0x11 || seg[13] != 0x11)
          return fail(IRX_JPEG_SAMPLING, "sampling other than 4:2:0");
      }
      for (int i = 0; i < nc; ++i)
        if (info->qsel[i] > 1) return fail(IRX_JPEG_TABLES, "quantisation table selector above 1");
      if (H < kMinSide || W < kMinSide) return fail(IRX_JPEG_SIZE, "H and W must be at least 8");
      info->H = H;
      info->W = W;
      info->ncomp = nc;
      have_sof = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
      return fail(IRX_JPEG_SOF, "progressive, extended, lossless or arithmetic coding");
    } else if (m == 0xDB) {
      for (long q = 0; q < sl; q += 65) {
        const int pq = seg[q] >> 4, tq = seg[q] & 15;
        if (pq != 0) return fail(IRX_JPEG_DQT16, "16-bit quantisation table");
        if (tq > 1) return fail(IRX_JPEG_TABLES, "quantisation table id above 1");
        if (q + 65 > sl) return fail(IRX_JPEG_MALFORMED, "short DQT");
        for (int k = 0; k < 64; ++k) {
          if (seg[q + 1 + k] == 0) return fail(IRX_JPEG_MALFORMED, "zero quantisation value");
          info->qt[tq][kZigzag[k]] = seg[q + 1 + k];
        }
      }
    } else if (m == 0xC4) {
      long q = 0;
      while (q < sl) {
        if (q + 17 > sl) return fail(IRX_JPEG_MALFORMED, "short DHT");
        const int tc = seg[q] >> 4, th = seg[q] & 15;
        if (tc > 1 || th > 1) return fail(IRX_JPEG_TABLES, "Huffman table class or id above 1");
        const uint8_t* bits = seg + q + 1;
        int cnt = 0;
        long code = 0;
        for (int l = 0; l < 16; ++l) {                       // the codes must fit their lengths, all-ones excluded
          cnt += bits[l];
          code += bits[l];
          if (code > (1L << (l + 1)) - 1) return fail(IRX_JPEG_MALFORMED, "over-subscribed Huffman table");
          code <<= 1;
        }
        if (cnt > 256 || q + 17 + cnt > sl) return fail(IRX_JPEG_MALFORMED, "short DHT");
        const uint8_t* vals = seg + q + 17;
        if (tc == 0) {
          if (cnt > 16) return fail(IRX_JPEG_TABLES, "DC category above 11");
          for (int i = 0; i < cnt; ++i)
            if (vals[i] > 11) return fail(IRX_JPEG_TABLES, "DC category above 11");
          std::memcpy(info->dc_bits[th], bits, 16);
          std::memset(info->dc_vals[th], 0, 16);
          std::memcpy(info->dc_vals[th], vals, cnt);
          info->dc_count[th] = cnt;
        } else {
          for (int i = 0; i < cnt; ++i)
            if ((vals[i] & 15) > 10) return fail(IRX_JPEG_TABLES, "AC size above 10");
          std::memcpy(info->ac_bits[th], bits, 16);
          std::memset(info->ac_vals[th], 0, 256);
          std::memcpy(info->ac_vals[th], vals, cnt);
          info->ac_count[th] = cnt;
        }
        q += 17 + cnt;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return fail(IRX_JPEG_MALFORMED, "DRI length");
      if (seg[0] || seg[1]) return fail(IRX_JPEG_DRI, "restart interval");
    } else if (m == 0xEE) {
      if (sl >= 5 && std::memcmp(seg, "Adobe", 5) == 0) return fail(IRX_JPEG_ADOBE, "Adobe APP14 marker");
    } else if (m == 0xDA) {
      if (!have_sof) return fail(IRX_JPEG_MALFORMED, "SOS before SOF0");
      const int nc = info->ncomp;
      if (sl < 1 || seg[0] != nc) return fail(IRX_JPEG_MULTISCAN, "a scan that does not hold every component");
      if (sl != 4 + 2 * nc) return fail(IRX_JPEG_MALFORMED, "SOS length");
      for (int i = 0; i < nc; ++i) {
        if (seg[1 + 2 * i] != comp_id[i]) return fail(IRX_JPEG_MALFORMED, "scan components out of frame order");
        const int dsel = seg[2 + 2 * i] >> 4, asel = seg[2 + 2 * i] & 15;
        if (dsel > 1 || asel > 1 || info->dc_count[dsel] == 0 || info->ac_count[asel] == 0)
          return fail(IRX_JPEG_TABLES, "scan names a Huffman table the file does not define");
        info->dcsel[i] = dsel;
        info->acsel[i] = asel;
      }
      if (seg[1 + 2 * nc] != 0 || seg[2 + 2 * nc] != 63 || seg[3 + 2 * nc] != 0)
        return fail(IRX_JPEG_SOF, "spectral selection or successive approximation");
      for (int i = 0; i < nc; ++i)
        if (info->qt[info->qsel[i]][0] == 0)
          return fail(IRX_JPEG_TABLES, "frame names a quantisation table the file does not define");
      break;
    }
    // everything else (APPn, COM, DNL, ...) is skipped
  }
  long e = p;
  for (;;) {
    const void* f = e < n ? std::memchr(d + e, 0xFF, (size_t)(n - e)) : nullptr;
    if (!f) return fail(IRX_JPEG_SCAN_CUT, "file ends in the scan");
    e = static_cast<const uint8_t*>(f) - d;
    if (e + 1 >= n) return fail(IRX_JPEG_SCAN_CUT, "file ends in the scan");
    if (d[e + 1] != 0) break;
    e += 2;
  }
  if (e == p) return fail(IRX_JPEG_MALFORMED, "empty scan");
  if (d[e + 1] >= 0xD0 && d[e + 1] <= 0xD7) return fail(IRX_JPEG_DRI, "restart marker in the scan");
  if (d[e + 1] != 0xD9) return fail(IRX_JPEG_MULTISCAN, "the scan is not followed by EOI");
  info->scan_off = p;
  info->scan_len = e - p;
  return 0;
}

}  // namespace

extern "C" int irx_jpeg_parse(const uint8_t* file, long len, irx_jpeg_info* info) {
  try {
    if (!info || len < 0 || (!file && len > 0)) return fail(IRX_JPEG_MALFORMED, "null pointer or negative length");
    return parse(file, len, info);
  } catch (const std::exception& e) {
    return fail(IRX_JPEG_MALFORMED, e.what());
  } catch (...) {
    return fail(IRX_JPEG_MALFORMED, "unknown error");
  }
}
