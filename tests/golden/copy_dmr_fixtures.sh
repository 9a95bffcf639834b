#!/bin/bash
# Provenance: DATA fixtures of nanoporetech/modkit v0.4.4's dmr regression test (tests/test_dmr.rs, test_dmr_regression): the regions BED
# it gives to `dmr pair -r` (six CpG islands of chr20; blank-separated, names that hold blanks) and the table it expects for the two lung
# tables that copy_bedmethyl_fixtures.sh brings, copied verbatim from the checkout's tests/resources.  The test's reference FASTA
# (GRCh38_chr20.fa) is not part of the checkout; tests/test_gpu_dmr_pair.py writes a stand-in.  No reference SOURCE code is copied.
set -e
SRC=${1:?usage: copy_dmr_fixtures.sh <modkit checkout>/tests/resources}
DST=$(dirname "$0")/modkit_fixtures
mkdir -p "$DST"
for f in cpg_chr20_with_orig_names_selection.bed test_output_chr20-2.bed; do
  cp "$SRC/$f" "$DST/$f"
done
echo "copied 2 files"
