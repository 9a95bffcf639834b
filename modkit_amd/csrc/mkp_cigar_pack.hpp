// The 16-bit CIGAR of the slot decoder (mkp_decode_slots, mkp_slots.hip): one uint16_t per op, (len << 4) | op — a BAM CIGAR word whose
// length fits 12 bits is its own low half.  Written next to cigar[] by both packers (ingest_copy_record, mkp_ingest_dev.hpp; Packer::add,
// mkp_pack.hpp), each read at an offset of its own that is a multiple of four entries, so that a lane's four ops are one aligned 8-byte
// load.  A read with an op longer than MKP_CIGAR16_MAX_LEN is marked MKP_RF_CIGW (mkp_device.h) and decoded from its 32-bit words: no op is
// ever split, op counts and indexes are the same in both arrays.  Plain C++ on both sides: tests/test_cigar_pack.py checks it against a model.
#pragma once
#include <stdint.h>

#ifndef MKP_HD
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MKP_HD __host__ __device__ __forceinline__
#else
#define MKP_HD static inline
#endif
#endif

#define MKP_CIGAR16_MAX_LEN 4095u

// the op's length fits the 16-bit form
MKP_HD bool mkp_cigar16_fits(uint32_t w) { return (w >> 4) <= MKP_CIGAR16_MAX_LEN; }
// the 16-bit form of a CIGAR word that fits (of one that does not: its low half — the read is flagged and the entry never decoded)
MKP_HD uint16_t mkp_cigar16_pack(uint32_t w) { return (uint16_t)((((w >> 4) & MKP_CIGAR16_MAX_LEN) << 4) | (w & 15u)); }
// ... and back to the BAM word
MKP_HD uint32_t mkp_cigar16_unpack(uint32_t e) { return (((e & 0xffffu) >> 4) << 4) | (e & 15u); }
// "this read has an op that does not fit": it keeps the 32-bit path (MKP_RF_CIGW)
MKP_HD bool mkp_cigar16_read_wide(const uint32_t* words, uint32_t n_cigar) {
  bool wide = false;
  for (uint32_t k = 0; k < n_cigar; k++) wide = wide || !mkp_cigar16_fits(words[k]);
  return wide;
}
// entries a read of n_cigar ops takes in the 16-bit array (every read starts on a multiple of four entries)
MKP_HD uint32_t mkp_cigar16_room(uint32_t n_cigar) { return (n_cigar + 3u) & ~3u; }
