// The base half of the slot decoder's plane (MKP_PLANE_WORDS in mkp_device.h): BAM 4-bit SEQ codes -> 2-bit base codes, 32 stored
// bases per plane entry.  Shared by the plane builder (mkp_call_plane, mkp_slots.hip) and the host test that checks the packing
// against a model (tests/test_base_pack.py), so it is plain C++ on both sides.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MKP_HD __host__ __device__ __forceinline__
#else
#define MKP_HD static inline
#endif

// One SEQ dword = stored bases 8 d .. 8 d + 7 (base 2j is the HIGH nibble of byte j).  Returns the 2-bit codes of its eight bases at bits
// 2k (A=0 C=1 G=2 T=3: the bit index of the one-hot BAM code, DnaBase::parse, mod_base_code.rs:188-196) and, at bit 16 + k, a flag for each
// base that is not A/C/G/T (a nibble that is not one-hot: N, IUPAC codes, '=', 0); a flagged base gets code 0.
MKP_HD uint32_t mkp_pack_bases8_all(uint32_t d) {
  const uint32_t x = ((d >> 4) & 0x0f0f0f0fu) | ((d & 0x0f0f0f0fu) << 4);   // nibble k = base k
  uint32_t p = x - ((x >> 1) & 0x55555555u);                              // set bits per nibble (0..4) ...
  p = (p & 0x33333333u) + ((p >> 2) & 0x33333333u);
  const uint32_t t = p ^ 0x11111111u;                                     // ... 0 where exactly one
  uint32_t b = (t | (t >> 1) | (t >> 2)) & 0x11111111u;                   // 1 bit at 4 k: not one-hot
  // one-hot 1, 2, 4, 8 -> 0, 1, 2, 3: bit 0 = C or T, bit 1 = G or T
  uint32_t c = ((((x >> 1) | (x >> 3)) & 0x11111111u) | (((x >> 1) | (x >> 2)) & 0x22222222u)) & ~(b * 3u);   // 2 bits at 4 k
  c = (c | (c >> 2)) & 0x0f0f0f0fu; c = (c | (c >> 4)) & 0x00ff00ffu; c = (c | (c >> 8)) & 0x0000ffffu;
  b = (b | (b >> 3)) & 0x03030303u; b = (b | (b >> 6)) & 0x000f000fu; b = (b | (b >> 12)) & 0x000000ffu;
  return c | (b << 16);
}

// The same for the first n_valid bases only: bases at or past n_valid (the pad nibble of an odd length, the dword's tail) give code 0
// and no flag.
MKP_HD uint32_t mkp_pack_bases8(uint32_t d, uint32_t n_valid) {
  const uint32_t r = mkp_pack_bases8_all(d);
  if (n_valid >= 8u) return r;
  return (r & ((1u << (2u * n_valid)) - 1u)) | (r & (((1u << n_valid) - 1u) << 16));
}

// One plane word = four SEQ dwords (stored bases 32 w .. 32 w + 31), n_valid = bases of the read in it (0..32).  Writes the codes of bases
// 0..15 to *lo and 16..31 to *hi (2 bits each) and returns the not-A/C/G/T flags (bit b = base 32 w + b).
MKP_HD uint32_t mkp_pack_bases32(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t n_valid, uint32_t* lo, uint32_t* hi) {
  const uint32_t p0 = mkp_pack_bases8_all(d0), p1 = mkp_pack_bases8_all(d1), p2 = mkp_pack_bases8_all(d2), p3 = mkp_pack_bases8_all(d3);
  uint32_t l = (p0 & 0xffffu) | (p1 << 16), h = (p2 & 0xffffu) | (p3 << 16);
  uint32_t bad = (p0 >> 16) | ((p1 >> 16) << 8) | ((p2 >> 16) << 16) | ((p3 >> 16) << 24);
  if (n_valid < 32u) {
    bad &= (1u << n_valid) - 1u;
    if (n_valid < 16u) { l &= (1u << (2u * n_valid)) - 1u; h = 0u; } else h &= (1u << (2u * (n_valid - 16u))) - 1u;
  }
  *lo = l; *hi = h;
  return bad;
}

// Bit b set where base b of a plane word is `code` (two 16-base halves of 2-bit codes, as mkp_pack_bases32 writes them); the caller masks
// out the bases that are not A/C/G/T or lie past the read (their code is 0).
MKP_HD uint32_t mkp_bases_eq(uint32_t lo, uint32_t hi, uint32_t code) {
  const uint32_t pat = code * 0x55555555u;
  uint32_t a = lo ^ pat, b = hi ^ pat;
  a = ~(a | (a >> 1)) & 0x55555555u; b = ~(b | (b >> 1)) & 0x55555555u;   // 1 bit at 2 k
  uint32_t e = a | (b << 1);                                               // base k at 2 k, base 16 + k at 2 k + 1
  // unshuffle: even bits -> low half, odd bits -> high half
  e = (e & 0x99999999u) | ((e >> 1) & 0x22222222u) | ((e << 1) & 0x44444444u);
  e = (e & 0xc3c3c3c3u) | ((e >> 2) & 0x0c0c0c0cu) | ((e << 2) & 0x30303030u);
  e = (e & 0xf00ff00fu) | ((e >> 4) & 0x00f000f0u) | ((e << 4) & 0x0f000f00u);
  e = (e & 0xff0000ffu) | ((e >> 8) & 0x0000ff00u) | ((e << 8) & 0x00ff0000u);
  return e;
}
