// mpjx_pack_plan.hpp — host-side planning of mpjx_pack / mpjx_unpack / mpjx_pack_size: the arithmetic of one
// mpjbuf section and the descriptor of k_pack (mpjx_k_pack.hip). No HIP include: plain C++17, compiled, tested
// and sanitized on the CPU (tests/cpp/pack_plan_test.cpp); the kernel includes the same header.
//
// One section of an mpjbuf static-buffer image (src/mpjbuf/Buffer.java:609-704, NIOBuffer.java:520-563):
//   h = round_up(position, 8)         byte h: mpjbuf type code (base type code - 1); h+1..h+3: zero;
//                                     h+4..h+7: big-endian int32 count of BASE elements (count * type.Size())
//   h + 8                             the elements in PACK order (mpjx_indexed_plan.hpp: item by item, blocks in
//                                     constructor order), each base word big-endian
//   end = h + 8 + words * word bytes  the position the call returns
// The count is a Java int: a section of more than 2^31 - 1 base elements does not exist.
//
// Granule. One lane of k_pack moves one granule of the packed stream, as in k_strided / k_indexed: the largest
// power of two <= 16 B that divides the buffer side's block bytes, strides, extent and base address and the
// payload's address (strided_granule_log over the layout and the contiguous payload). It never falls below the
// base word: the buffer is element-aligned, a layout's offsets and lengths are whole elements, and the payload
// starts at image + h + 8 with image 8-byte aligned and h a multiple of 8. So every granule holds whole words,
// the swap is done in registers per granule, and no byte path exists (plan_pack_seg asserts it).
#pragma once
#include <assert.h>
#include <string.h>

#include "mpjx_indexed_plan.hpp"

namespace mpjx {

constexpr int64_t kPackMaxWords = 0x7fffffff;  // the header's count field is a Java int

// Comm.Pack_size, padding quirk included (src/mpi/BasicType.java:209-220, the same in Contiguous, Vector and
// Indexed): t = 8 + count * byteSize, plus t % 8 (not 8 - t % 8). An upper bound of what mpjx_pack writes
// only for a section that starts at a multiple of 8.
inline int64_t pack_size_bytes(int64_t count, int64_t item_bytes) {
  const int64_t t = 8 + count * item_bytes;
  return t + t % 8;
}

struct PackSection {
  int64_t h = 0;      // the header's position: round_up(position, 8)
  int64_t pay = 0;    // the payload's position: h + 8
  int64_t end = 0;    // one past the payload: the position returned
  int64_t words = 0;  // base elements: count * type.Size()
};

// The section of `count` items of `size` base elements of `bsz` bytes at `position` of an image of image_bytes.
// False with *err set for a negative count or position, more than 2^31 - 1 base elements, or a section that
// would end past image_bytes.
inline bool plan_pack_section(int64_t position, int64_t count, int64_t size, int bsz, int64_t image_bytes,
                              PackSection* out, std::string* err) {
  *out = PackSection{};
  if (count < 0 || position < 0 || image_bytes < 0) {
    *err = std::string("negative ") + (count < 0 ? "count " + std::to_string(count)
                                       : position < 0 ? "position " + std::to_string(position)
                                                      : "image size " + std::to_string(image_bytes));
    return false;
  }
  if (size > 0 && count > kPackMaxWords / size) {
    *err = std::to_string(count) + " items of " + std::to_string(size) +
           " base elements exceed the section header's int32 count (2^31 - 1)";
    return false;
  }
  out->words = count * size;
  const int64_t payload = out->words * bsz;  // < 2^34
  // position + 8 <= image_bytes keeps position + 7 from overflowing; h + 8 <= image_bytes does the same for pay
  if (image_bytes < 8 || position > image_bytes - 8 || image_bytes - (position + 7) / 8 * 8 < 8) {
    *err = "the section header at position " + std::to_string(position) + " ends past the image of " +
           std::to_string(image_bytes) + " bytes";
    return false;
  }
  out->h = (position + 7) / 8 * 8;
  out->pay = out->h + 8;
  if (image_bytes - out->pay < payload) {
    *err = "the section (header at " + std::to_string(out->h) + ", " + std::to_string(payload) +
           " payload bytes) ends past the image of " + std::to_string(image_bytes) + " bytes";
    return false;
  }
  out->end = out->pay + payload;
  return true;
}

// The 8 header bytes as the 64-bit word a little-endian device stores at h
inline uint64_t pack_header_word(int base, int64_t words) {
  const uint32_t n = (uint32_t)words;
  const unsigned char b[8] = {(unsigned char)(base - 1), 0, 0, 0, (unsigned char)(n >> 24), (unsigned char)(n >> 16),
                              (unsigned char)(n >> 8), (unsigned char)n};
  uint64_t w;
  memcpy(&w, b, 8);
  return w;
}

// What k_pack reads. The buffer side is k_indexed's side (regular or irregular); the payload side is linear.
struct PackSeg {
  IndexedSide lay;  // the buffer's layout: item 0's origin, lb not subtracted
  uint64_t pay;     // byte address of the payload (image + h + 8)
  uint64_t hdr;     // byte address of the header (image + h)
  uint64_t header;  // pack: the header word to store
  int64_t words;    // unpack: the base elements the header must announce
  int64_t room;     // unpack: bytes from the payload's start to the end of the image
  int* status;      // unpack: device-accessible int, receives MPJX_MPJBUF_* for a malformed header
  uint32_t ngran;   // granules of the packed stream (0: header only)
  uint32_t glog;    // log2 of the granule: wlog..4
  uint32_t wlog;    // log2 of the base word: 0..3
  uint32_t lin;     // the buffer side is one contiguous run: its address is linear too
  int code;         // the mpjbuf type code: base type code - 1
};

inline SideBytes packed_side(uint64_t addr, int64_t bytes) {
  SideBytes x;
  x.base = addr;
  x.bb = x.sb = x.eb = bytes;
  x.nb = x.items = 1;
  return x;
}

// The descriptor of one section: `lay` (plan_side of the type over the buffer; its total is the payload's) with
// its device table `tab` (irregular layouts only), the image at byte address `image`.
inline void plan_pack_seg(const SideBytes& lay, const IdxEnt* tab, uint64_t image, int64_t image_bytes,
                          const PackSection& sec, int base, int bsz, int* status, PackSeg* out) {
  const int64_t payload = sec.words * bsz;
  assert(lay.total() == payload || payload == 0);
  const SideBytes pay = packed_side(image + (uint64_t)sec.pay, payload);
  *out = PackSeg{};
  out->pay = pay.base;
  out->hdr = image + (uint64_t)sec.h;
  out->header = pack_header_word(base, sec.words);
  out->words = sec.words;
  out->room = image_bytes - sec.pay;
  out->status = status;
  out->code = base - 1;
  while ((1 << out->wlog) < bsz) out->wlog++;
  out->glog = out->wlog;
  if (payload == 0) return;  // header only: the buffer is not touched
  const uint32_t g = strided_granule_log(lay, pay);
  assert((1 << g) >= bsz && "element-aligned buffer, 8-aligned payload, whole-element layout");
  IndexedSeg sg;
  std::string err;
  // below 2^32 granules: at most 2^31 - 1 words of at most one granule each
  const int rc = plan_indexed_seg(lay, tab, pay, nullptr, &sg, &err);
  assert(rc == kTypeOk && sg.glog == g);
  (void)rc;
  out->lay = sg.s;
  out->ngran = sg.ngran;
  out->glog = g;
  out->lin = lay.contiguous() ? 1u : 0u;
}

// The byte address of packed granule q on the buffer side, as k_pack computes it (the table searched where it
// lies); the payload side is pay + (q << glog).
MPJX_HD inline uint64_t pack_lay_addr(const PackSeg& a, uint32_t q) {
  if (a.lin) return a.lay.r.base + ((uint64_t)q << a.glog);
  return indexed_addr(a.lay, q, a.glog);
}

}  // namespace mpjx
