// The grammar of one bedMethyl line (BedMethylLine, src/dmr/bedmethyl.rs:40-86), the one copy of it: the host reader (mkp_bedmethyl_in.hpp)
// and the device reader (mkp_bedmethyl_parse, mkp_bedmethyl.hip) both call mkp_bedmethyl_parse_line.  Plain C++ on both sides:
// tests/test_bedmethyl_line_host.py checks it against the model of tests/bedmethyl_merge_model.py.
//
// A line (without its '\n'; one '\r' at its end is dropped) holds 18 or more fields separated by runs of tabs and / or blanks.  Field 1
// chrom, 2 start, 3 end, 4 name — the mod code is the name up to its first comma: one character, or a ChEBI number <= 2^31 - 1 —, 5 score =
// valid_coverage, 6 strand (+ - .), 12-18 the seven other counts; fields 2, 3, 5, 7, 8, 10 and 12-18 are decimal and <= 2^32 - 1.  The
// fields are checked in their order on the line, a field's characters from left to right, after the field count: the first finding is
// the one returned.
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

// what mkp_bedmethyl_parse_line returns: 0, or (status class << 8) | field number (1-based; of MKP_BML_FEW_FIELDS: the fields found)
#define MKP_BML_FEW_FIELDS 1u   // fewer than 18 fields
#define MKP_BML_NOT_NUMBER 2u   // a decimal field is not one
#define MKP_BML_BEYOND_32 3u    // a decimal field is beyond 2^32 - 1
#define MKP_BML_BAD_CODE 4u     // the name is neither one character nor a ChEBI number <= 2^31 - 1
#define MKP_BML_BAD_STRAND 5u   // the strand is none of + - .
#define MKP_BML_CLASS(code) ((code) >> 8)
#define MKP_BML_FIELD(code) ((code) & 0xffu)

struct MkpBedLine {
  uint32_t chrom_off, chrom_len;   // the chrom's bytes inside the line
  uint32_t pos, code;              // code: the character, or 0x80000000 | ChEBI number (ModCodeRepr, as the rows carry it)
  uint32_t strand;                 // 0 '+', 1 '-', 2 '.'
  uint32_t n_valid, n_mod, n_canonical, n_other, n_delete, n_fail, n_diff, n_nocall;
};

MKP_HD bool mkp_bml_sep(uint8_t c) { return c == ' ' || c == '\t'; }
// the next field [*s, *e) at or behind *i; false = the line has no further field
MKP_HD bool mkp_bml_field(const uint8_t* line, uint32_t len, uint32_t* i, uint32_t* s, uint32_t* e) {
  uint32_t p = *i;
  while (p < len && mkp_bml_sep(line[p])) p++;
  *s = p;
  while (p < len && !mkp_bml_sep(line[p])) p++;
  *e = p; *i = p;
  return *e > *s;
}
// the decimal field [s, e) (not empty); *err takes the first finding of the line
MKP_HD uint32_t mkp_bml_number(const uint8_t* line, uint32_t s, uint32_t e, uint32_t field, uint32_t* err) {
  uint64_t v = 0;
  for (uint32_t i = s; i < e; i++) {
    const uint8_t c = line[i];
    if (c < '0' || c > '9') { if (!*err) *err = (MKP_BML_NOT_NUMBER << 8) | field; return 0u; }
    v = v * 10u + (uint64_t)(c - '0');
    if (v > 0xffffffffull) { if (!*err) *err = (MKP_BML_BEYOND_32 << 8) | field; return 0u; }
  }
  return (uint32_t)v;
}
// ModCodeRepr::parse (src/mod_base_code.rs:112-122) of the name [s, e) up to its first comma; 0 = not a code
MKP_HD uint32_t mkp_bml_code(const uint8_t* line, uint32_t s, uint32_t e) {
  uint32_t ce = s;
  while (ce < e && line[ce] != ',') ce++;
  if (ce - s == 1u) return (uint32_t)line[s];
  if (ce == s) return 0u;
  uint64_t v = 0;
  for (uint32_t i = s; i < ce; i++) {
    if (line[i] < '0' || line[i] > '9') return 0u;
    v = v * 10u + (uint64_t)(line[i] - '0');
    if (v > 0x7fffffffull) return 0u;
  }
  return 0x80000000u | (uint32_t)v;
}

// line[0, len): one line without its '\n'.  0 and *out filled, or the code of the first finding (*out is then unspecified).
MKP_HD uint32_t mkp_bedmethyl_parse_line(const uint8_t* line, uint32_t len, MkpBedLine* out) {
  if (len && line[len - 1u] == '\r') len--;
  uint32_t i = 0, s = 0, e = 0, err = 0;
#define MKP_BML_NEXT(k) if (!mkp_bml_field(line, len, &i, &s, &e)) return (MKP_BML_FEW_FIELDS << 8) | ((k) - 1u)
  MKP_BML_NEXT(1u); out->chrom_off = s; out->chrom_len = e - s;
  MKP_BML_NEXT(2u); out->pos = mkp_bml_number(line, s, e, 2u, &err);
  MKP_BML_NEXT(3u); (void)mkp_bml_number(line, s, e, 3u, &err);
  MKP_BML_NEXT(4u); out->code = mkp_bml_code(line, s, e); if (!out->code && !err) err = (MKP_BML_BAD_CODE << 8) | 4u;
  MKP_BML_NEXT(5u); out->n_valid = mkp_bml_number(line, s, e, 5u, &err);
  MKP_BML_NEXT(6u);
  { const uint8_t c = line[s]; const bool one = e - s == 1u;
    out->strand = c == '+' ? 0u : c == '-' ? 1u : 2u;
    if ((!one || (c != '+' && c != '-' && c != '.')) && !err) err = (MKP_BML_BAD_STRAND << 8) | 6u; }
  MKP_BML_NEXT(7u); (void)mkp_bml_number(line, s, e, 7u, &err);
  MKP_BML_NEXT(8u); (void)mkp_bml_number(line, s, e, 8u, &err);
  MKP_BML_NEXT(9u);
  MKP_BML_NEXT(10u); (void)mkp_bml_number(line, s, e, 10u, &err);
  MKP_BML_NEXT(11u);
  MKP_BML_NEXT(12u); out->n_mod = mkp_bml_number(line, s, e, 12u, &err);
  MKP_BML_NEXT(13u); out->n_canonical = mkp_bml_number(line, s, e, 13u, &err);
  MKP_BML_NEXT(14u); out->n_other = mkp_bml_number(line, s, e, 14u, &err);
  MKP_BML_NEXT(15u); out->n_delete = mkp_bml_number(line, s, e, 15u, &err);
  MKP_BML_NEXT(16u); out->n_fail = mkp_bml_number(line, s, e, 16u, &err);
  MKP_BML_NEXT(17u); out->n_diff = mkp_bml_number(line, s, e, 17u, &err);
  MKP_BML_NEXT(18u); out->n_nocall = mkp_bml_number(line, s, e, 18u, &err);
#undef MKP_BML_NEXT
  return err;
}
