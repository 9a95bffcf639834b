// Internal (not installed): the host-only steps of the device ingest (mkp_ingest_host.cpp runs them between its launches).  Plain
// arithmetic over the ingest plan, the upload layout and the tables the chain kernels wrote: no HIP header is read here and no HIP call is
// made — g++ compiles it with mkp_pack.hpp and mkp_ingest_dev.hpp (MKP_INGEST_HOST_SHIM) behind it, and tests/ingest_emul.cpp drives the
// same functions over its emulated kernels.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "mkp_ingest_dev.hpp"
#include "mkp_pack.hpp"

namespace mkp {

// ---- upload layout.  The window's file ranges lie one behind the other in the upload buffer, each 64-byte aligned (zbase); they go up in
// PIECES of at most `piece_bytes`, `slots` pieces to a ROUND; round_end_z[r] = where round r's bytes end in the buffer.
constexpr size_t kIngestPiece = (size_t)1 << 20, kIngestSlots = 16;   // the product's piece (also the width of a staging slot) and round
struct UploadPiece { uint64_t file_off, z_off; size_t n; };
struct UploadCopy { size_t k; uint64_t z_off; size_t bytes; };   // pieces from slot k of the round's staging half on: one copy to z_off
struct UploadLayout {
  std::vector<uint64_t> zbase; uint64_t zbytes = 0;
  std::vector<UploadPiece> pieces; size_t slots = 1, n_rounds = 0;
  std::vector<uint64_t> round_end_z;
  static UploadLayout of(const std::vector<BamSource::IngestRange>& ranges, size_t piece_bytes, size_t slots) {
    UploadLayout u; u.slots = slots; u.zbase.resize(ranges.size());
    for (size_t r = 0; r < ranges.size(); r++) { u.zbase[r] = u.zbytes; u.zbytes += (ranges[r].file_len + 63) & ~63ull; }
    for (size_t r = 0; r < ranges.size(); r++) for (uint64_t o = 0; o < ranges[r].file_len; o += piece_bytes)
      u.pieces.push_back({ranges[r].file_off + o, u.zbase[r] + o, (size_t)std::min<uint64_t>(piece_bytes, ranges[r].file_len - o)});
    u.n_rounds = (u.pieces.size() + slots - 1) / slots;
    u.round_end_z.assign(u.n_rounds, u.zbytes);
    for (size_t r = 0; r + 1 < u.n_rounds; r++) { const UploadPiece& last = u.pieces[(r + 1) * slots - 1]; u.round_end_z[r] = last.z_off + last.n; }
    return u;
  }
  size_t round_pieces(size_t round) const { return std::min(slots, pieces.size() - round * slots); }
  // one copy per run of pieces that lie back to back in the staging half (a slot is `slot_bytes` wide) AND in the window (a whole round,
  // for a window of one file range): 2 MiB copies do not reach the link's rate, 32 MiB ones do
  std::vector<UploadCopy> copies(size_t round, size_t slot_bytes) const {
    std::vector<UploadCopy> out; const size_t p0 = round * slots, n = round_pieces(round);
    for (size_t k = 0; k < n;) {
      size_t k1 = k + 1, bytes = pieces[p0 + k].n;
      while (k1 < n && pieces[p0 + k1 - 1].n == slot_bytes && pieces[p0 + k1].z_off == pieces[p0 + k1 - 1].z_off + slot_bytes) {
        bytes += pieces[p0 + k1].n; k1++; }
      out.push_back({k, pieces[p0 + k].z_off, bytes});
      k = k1;
    }
    return out;
  }
};

// ---- chain table: the chains of the plan as positions in the upload buffer (what the chain kernels read); chain_zend[i]: chain i reads
// nothing at or behind this
inline void ingest_chain_table(const BamSource::IngestPlan& plan, const std::vector<BamSource::IngestChain>& chains,
    const std::vector<uint64_t>& zbase, MkpZChain* zc, std::vector<uint64_t>* chain_zend) {
  chain_zend->resize(chains.size());
  for (size_t i = 0; i < chains.size(); i++) { const BamSource::IngestRange& rg = plan.ranges[chains[i].range];
    const uint64_t zb = zbase[chains[i].range], fo = rg.file_off;
    MkpZChain c; c.start = zb + (chains[i].start - fo); c.stop = chains[i].stop == UINT64_MAX ? ~0ull : zb + (chains[i].stop - fo);
      c.range_end = zb + rg.file_len;
    c.ce = (rg.vend >> 16) >= fo ? zb + ((rg.vend >> 16) - fo) : 0; c.ue = (uint32_t)(rg.vend & 0xffff); c.pad = 0; zc[i] = c;
    (*chain_zend)[i] = c.stop == ~0ull ? c.range_end : std::min<uint64_t>(c.stop, c.range_end); }
}

// ---- stage cut: a stage that begins at chain c0 and took the rounds up to one ending at z_end holds the chains that end inside them
// (every chain left, with the last round); returns the chain the next stage begins at
inline size_t ingest_stage_cut(const std::vector<uint64_t>& chain_zend, size_t c0, uint64_t z_end, bool last_round) {
  size_t c1 = c0; while (c1 < chain_zend.size() && (last_round || chain_zend[c1] <= z_end)) c1++;
  return c1;
}

// The stages as they were cut: stage j = chains [c0[j], c0[j + 1]) and nblk[j] blocks; its counts lie at cnt_all + c0[j] + j (as offsets
// once scanned, the total behind them), its MkpZBlk entries behind those of the stages before it.
struct IngestStages {
  std::vector<size_t> c0{0}; std::vector<uint32_t> nblk;
  size_t size() const { return nblk.size(); }
  size_t cnt_at(size_t j) const { return c0[j] + j; }
};
// ---- the per-chain block lists (file offsets, what BamSource::ingest_layout reads) from the appended table
inline std::vector<std::vector<BamSource::IngestBlk>> ingest_chain_blocks(const BamSource::IngestPlan& plan,
    const std::vector<BamSource::IngestChain>& chains, const std::vector<uint64_t>& zbase, const IngestStages& st, const uint32_t* cnt_all,
    const MkpZBlk* zb) {
  std::vector<std::vector<BamSource::IngestBlk>> parts(chains.size());
  size_t base = 0;
  for (size_t j = 0; j < st.size(); j++) { const size_t c0 = st.c0[j], c1 = st.c0[j + 1]; const uint32_t* cb = cnt_all + st.cnt_at(j);
    for (size_t i = c0; i < c1; i++) { const uint64_t zbs = zbase[chains[i].range], fo = plan.ranges[chains[i].range].file_off;
      parts[i].reserve(cb[i - c0 + 1] - cb[i - c0]);
      for (uint32_t k = cb[i - c0]; k < cb[i - c0 + 1]; k++) { const MkpZBlk& z = zb[base + k];
        parts[i].push_back({fo + (z.coff - zbs), z.hdr, z.clen, z.isize, 0}); } }
    base += st.nblk[j]; }
  return parts;
}

// ---- the inflate's table of a whole laid-out window
inline std::vector<MkpBgzfBlock> ingest_window_blocks(const BamSource::IngestPlan& plan, const std::vector<uint64_t>& zbase,
    const std::string& path) {
  std::vector<MkpBgzfBlock> blks(plan.blks.size());
  for (size_t r = 0; r < plan.ranges.size(); r++) for (size_t k = plan.ranges[r].blk0; k < plan.ranges[r].blk1; k++) {
    const BamSource::IngestBlk& b = plan.blks[k];
    if (b.isize > 65536u) throw Error(MKP_E_IO, "BGZF block inflates to more than 64 KiB in " + path);
    blks[k] = {zbase[r] + (b.coff - plan.ranges[r].file_off) + b.hdr, b.doff, b.clen, b.isize};
  }
  return blks;
}

// ---- the page-locked small buffer of one window: block table and segments on their way up; totals, the status words as the CRC left
// them and as the decoders left them on their way down (offsets in bytes; the last three regions 64-byte aligned behind the segments)
struct SmallCarve {
  size_t blk = 0, seg = 0, tot = 0, stat = 0, stat0 = 0, need = 0;
  static SmallCarve of(size_t nb, size_t ns) {
    SmallCarve c; c.seg = nb * sizeof(MkpBgzfBlock); c.tot = c.seg + ns * sizeof(MkpSeg);
    c.stat = c.tot + ((sizeof(MkpIngestTotals) + 63) & ~(size_t)63); c.stat0 = c.stat + ((nb * 4 + 63) & ~(size_t)63);
    c.need = nb * sizeof(MkpBgzfBlock) + ns * sizeof(MkpSeg) + 2 * (nb * 4 + 64) + sizeof(MkpIngestTotals) + 256;
    return c;
  }
};

// ---- error bits of the record kernels -> the Error the host path would throw
inline void ingest_throw_error_bits(uint32_t err, const std::string& path) {
  if (err & MKP_IE_TRUNCATED) throw Error(MKP_E_IO, "truncated BAM record at the end of " + path);
  if (err & MKP_IE_CORRUPT) throw Error(MKP_E_IO, "corrupt BAM record");
  if (err & MKP_IE_CHAIN) throw Error(MKP_E_IO,
      "the BAM index does not match the file (a record chain misses an indexed record start): " + path + ".bai");
  if (err & (MKP_IE_TABLE | MKP_IE_4G)) throw Error(MKP_E_UNSUPPORTED, "shard exceeds 4 GiB of packed bases; use smaller shards");
  if (err & MKP_IE_QLEN) throw Error(MKP_E_INVALID, "CIGAR query length does not match SEQ length");
  if (err & MKP_IE_SPAN) throw Error(MKP_E_UNSUPPORTED,
      "a read or its alignment spans 2^26 bases or more (the depth walk packs query offsets in 27 bits)");
  if (err & MKP_IE_NONASCII) throw Error(MKP_E_UNSUPPORTED, "non-ASCII mod code");
  if (err & MKP_IE_CODES) throw Error(MKP_E_UNSUPPORTED, "more than 4 mod codes in one MM tag");
  if (err & MKP_IE_TAGS) throw Error(MKP_E_UNSUPPORTED, "more than 8 MM tags in one read");
}

inline uint64_t ingest_fnv64(const std::string& s) { uint64_t h = 1469598103934665603ull; for (unsigned char ch : s) { h ^= ch; h *= 1099511628211ull; } return h;
}

// ---- digest -> what the planner reads: name hashes, window indices, flags, and the layout id of every packed record (ids of `layouts`,
// this shard's own table).  S.hdr holds the n kept records' headers, S.so_hdr the n_so sampler-only ones, dig their digests in that order.
// A structure not seen in this shard yet: info_of(window index) gives its record's MkpRecInfo and bytes_of(info, &buf) the record from its
// block_size word on (bs + 4 bytes); it goes through the host packer, which interns the layout — and must arrive at the same key: a
// colliding hash would otherwise attach the wrong caller tables.
template <class InfoOf, class BytesOf>
inline void ingest_intern_layouts(ShardHost& S, Packer& layouts, const std::vector<MkpRecDigest>& dig, uint32_t n, uint32_t n_so,
    uint32_t n_all, InfoOf info_of, BytesOf bytes_of) {
  const uint32_t n_pk = n + n_so;
  S.name_hash.resize(n); S.dev_sum2.resize(n); S.dev_name_hash2.resize(n); S.dev_win_idx.resize(n); S.so_name_hash.resize(n_so);
    S.so_name_hash2.resize(n_so); S.so_win_idx.resize(n_so);
  std::unordered_map<uint64_t, uint16_t> by_hash; std::vector<uint8_t> recbuf;
  uint64_t ev_cap = 0, last_hash = 0; uint16_t last_id = 0; bool have_last = false;
  for (uint32_t j = 0; j < n_pk; j++) {
    const bool so = j >= n;
    MkpReadHdr& h = so ? S.so_hdr[j - n] : S.hdr[j];
    if (so) { S.so_name_hash[j - n] = dig[j].name_hash; S.so_name_hash2[j - n] = dig[j].name_hash2; S.so_win_idx[j - n] = (uint32_t)dig[j].win_idx;
      h.cigar16_off &= ~3u; }
    else { S.name_hash[j] = dig[j].name_hash; S.dev_name_hash2[j] = dig[j].name_hash2; S.dev_win_idx[j] = (uint32_t)dig[j].win_idx;
      S.dev_sum2[j] = (uint8_t)(h.cigar16_off & 1u); h.cigar16_off &= ~3u; ev_cap += h.event_cap; }
    if (!h.n_tags || (h.flags & MKP_RF_BAD)) continue;
    if (have_last && dig[j].key_hash == last_hash) { h.layout = last_id; continue; }   // (runs of one structure: most of a file)
    auto it = by_hash.find(dig[j].key_hash);
    if (it == by_hash.end()) {
      const uint64_t wi = dig[j].win_idx;
      if (wi >= n_all) throw Error(MKP_E_DEVICE, "internal: device ingest digest points at a record it did not pack");
      const MkpRecInfo ri = info_of(wi);
      if (ri.kind != 1 && ri.kind != 3) throw Error(MKP_E_DEVICE, "internal: device ingest digest points at a record it did not pack");
      bytes_of(ri, &recbuf);
      mkp_record r; const uint8_t* c = recbuf.data() + 4;
      memcpy(&r.tid, c, 4); memcpy(&r.pos, c + 4, 4); r.l_qname = c[8]; uint16_t nc; memcpy(&nc, c + 12, 2); r.n_cigar = nc;
        memcpy(&r.flag, c + 14, 2); memcpy(&r.l_qseq, c + 16, 4);
      r.l_data = (int32_t)ri.bs - 32; r.data = c + 32;
      ShardHost scratch; scratch.tid = S.tid;
      const size_t before = layouts.layouts.size();
      layouts.add(r, scratch);
      if (scratch.hdr.size() != 1 || (scratch.hdr[0].flags & MKP_RF_BAD) || !scratch.hdr[0].n_tags) throw Error(MKP_E_DEVICE,
          "internal: device and host tokenisers disagree on a record's tags");
      const uint16_t id = scratch.hdr[0].layout;
      if (ingest_fnv64(layouts.layout_keys[id]) != dig[j].key_hash) throw Error(MKP_E_DEVICE,
          "internal: device and host tokenisers disagree on a record's MM header structure");
      if (id < before) throw Error(MKP_E_DEVICE, "internal: two MM header structures share a 64-bit key hash");
      it = by_hash.emplace(dig[j].key_hash, id).first;
    }
    h.layout = it->second; last_hash = dig[j].key_hash; last_id = it->second; have_last = true;
  }
  S.n_events_cap = ev_cap;
}

}  // namespace mkp
