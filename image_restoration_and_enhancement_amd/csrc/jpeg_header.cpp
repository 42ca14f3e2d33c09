// The bytes of a baseline 4:2:0 JPEG file in front of its scan, as PIL.Image.save(f, "JPEG") writes them for an RGB
// image: SOI, APP0 (JFIF 1.1, density 1 x 1), two DQT (zigzag order), SOF0, four DHT (DC0, AC0, DC1, AC1; the
// Annex K tables) and SOS.  Host only, plain C++ (no HIP); jpeg_host.header is the same bytes in numpy.
#include <algorithm>
#include <exception>
#include <string>
#include <vector>

#include "../../include/irx.h"
#include "jpeg_tables.h"

namespace irx {
void set_error(const std::string& msg);   // capi.cpp
}

namespace {

using namespace irx::jpegtab;

int fail(const std::string& msg) {
  irx::set_error("irx_jpeg_header: " + msg);
  return -1;
}

void put16(std::vector<uint8_t>& v, int x) {
  v.push_back((uint8_t)(x >> 8));
  v.push_back((uint8_t)x);
}

void dht(std::vector<uint8_t>& v, int tc_th, const uint8_t* bits, const uint8_t* vals, int nvals) {
  v.push_back(0xFF);
  v.push_back(0xC4);
  put16(v, 19 + nvals);
  v.push_back((uint8_t)tc_th);
  v.insert(v.end(), bits, bits + 16);
  v.insert(v.end(), vals, vals + nvals);
}

}  // namespace

extern "C" int irx_jpeg_header(int H, int W, const int* qtables, uint8_t* buf, int cap) {
  try {
    if (!qtables || !buf) return fail("null pointer");
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return fail("H and W must be in 1..65535");
    for (int i = 0; i < 128; ++i)
      if (qtables[i] < 1 || qtables[i] > 255) return fail("quantisation table entries must be in 1..255 (baseline)");
    std::vector<uint8_t> v = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int t = 0; t < 2; ++t) {
      v.insert(v.end(), {0xFF, 0xDB, 0, 67, (uint8_t)t});
      for (int k = 0; k < 64; ++k) v.push_back((uint8_t)qtables[t * 64 + kZigzag[k]]);
    }
    v.insert(v.end(), {0xFF, 0xC0, 0, 17, 8});
    put16(v, H);
    put16(v, W);
    v.insert(v.end(), {3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    dht(v, 0x00, kDcBits[0], kDcVals, 12);
    dht(v, 0x10, kAcBits[0], kAcVals[0], 162);
    dht(v, 0x01, kDcBits[1], kDcVals, 12);
    dht(v, 0x11, kAcBits[1], kAcVals[1], 162);
    v.insert(v.end(), {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0});
    if ((int)v.size() > cap) return fail("buffer of " + std::to_string(cap) + " bytes, need " + std::to_string(v.size()));
    std::copy(v.begin(), v.end(), buf);
    return (int)v.size();
  } catch (const std::exception& e) {
    return fail(e.what());
  } catch (...) {
    return fail("unknown error");
  }
}
