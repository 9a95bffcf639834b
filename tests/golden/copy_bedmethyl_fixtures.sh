#!/bin/bash
# Provenance: DATA fixtures of nanoporetech/modkit v0.4.4's dmr tests (tests/test_dmr.rs): the two bgzip-compressed, tabix-indexed
# bedMethyl tables of one lung sample (adjacent normal / primary tumour, chr20, CpG, 5mC + 5hmC), copied verbatim from the checkout's
# tests/resources.  They are what `bedmethyl merge` reads in practice: BGZF, mixed delimiters (tabs up to column 10, blanks behind).
# The .tbi files are not copied: the readers here neither need nor read them.  No reference SOURCE code is copied.
set -e
SRC=${1:?usage: copy_bedmethyl_fixtures.sh <modkit checkout>/tests/resources}
DST=$(dirname "$0")/modkit_fixtures
mkdir -p "$DST"
for t in adjacent-normal primary-tumour; do
  f=lung_00733-m_${t}_5mc-5hmc_chr20_cpg_pileup.bed.gz
  cp "$SRC/$f" "$DST/$f"
done
echo "copied 2 files"
