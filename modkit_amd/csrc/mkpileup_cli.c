/* mkpileup — command-line front end of libmkpileup: `mkpileup pileup in.bam out.bed [modkit pileup flags]`,
 * `mkpileup pileup-hemi in.bam -o out.bed [modkit pileup-hemi flags]`, `mkpileup extract calls in.bam out.tsv [flags]`,
 * `mkpileup bedmethyl merge a.bed b.bed [c.bed ..] -g sizes.tsv -o out.bed [--force] [--bgzf]`,
 * `mkpileup dmr pair -a a.bed -b b.bed -r regions.bed --ref ref.fa --base C [-o out.bed] [flags of the region form of modkit dmr pair]`,
 * `mkpileup dmr sites -a a.bed -b b.bed --ref ref.fa --base C [-o out.bed] [flags of modkit dmr pair without -r]`,
 * `mkpileup dmr replicates -a a1.bed -a a2.bed .. -b b1.bed -b b2.bed .. --ref ref.fa --base C [-o out.bed] [the flags of dmr sites]`. */
#include <stdio.h>
#include <string.h>
#include "mkpileup.h"
int main(int argc, char** argv) {
  char err[1024] = {0};
  const int hemi = argc >= 2 && strcmp(argv[1], "pileup-hemi") == 0;
  const int extract = argc >= 3 && strcmp(argv[1], "extract") == 0 && strcmp(argv[2], "calls") == 0;
  if (argc >= 3 && strcmp(argv[1], "bedmethyl") == 0 && strcmp(argv[2], "merge") == 0) {
    int rc = mkp_bedmethyl_merge_main(argc - 3, (const char* const*)(argv + 3), NULL, NULL, err, sizeof(err));
    if (rc != MKP_OK) { fprintf(stderr, "Error! %s (status %d)\n", err, rc); return 1; }
    return 0;
  }
  if (argc >= 3 && strcmp(argv[1], "dmr") == 0) {
    int rc = MKP_E_UNSUPPORTED;
    if (strcmp(argv[2], "pair") == 0) rc = mkp_dmr_pair_main(argc - 3, (const char* const*)(argv + 3), NULL, err, sizeof(err));
    else if (strcmp(argv[2], "sites") == 0) rc = mkp_dmr_sites_main(argc - 3, (const char* const*)(argv + 3), NULL, err, sizeof(err));
    else if (strcmp(argv[2], "replicates") == 0) rc = mkp_dmr_reps_main(argc - 3, (const char* const*)(argv + 3), NULL, err, sizeof(err));
    else snprintf(err, sizeof(err), "dmr %s is not offered: only `dmr pair` over the regions of -r", argv[2]);
    if (rc != MKP_OK) { fprintf(stderr, "Error! %s (status %d)\n", err, rc); return 1; }
    return 0;
  }
  if (extract) {
    int rc = mkp_extract_calls_main(argc - 3, (const char* const*)(argv + 3), err, sizeof(err));
    if (rc != MKP_OK) { fprintf(stderr, "Error! %s (status %d)\n", err, rc); return 1; }
    return 0;
  }
  if (argc < 2 || (!hemi && strcmp(argv[1], "pileup") != 0)) {
    fprintf(stderr, "usage: mkpileup pileup <in.bam> <out.bed> [flags of `modkit pileup`] [--device N] [--stats]\n"
                    "       mkpileup pileup-hemi <in.bam> -o <out.bed> [flags of `modkit pileup-hemi`] [--device N] [--stats]\n"
                    "       mkpileup extract calls <in.bam> <out.tsv> [flags of `modkit extract calls`] [--device N] [--stats]\n"
                    "       mkpileup bedmethyl merge <a.bed> <b.bed> [..] -g <sizes.tsv> -o <out.bed> [--force] [--bgzf] [--device N] [--stats]\n"
                    "       mkpileup dmr pair -a <a.bed[.gz]> -b <b.bed[.gz]> -r <regions.bed> --ref <ref.fa> --base C [--base A ..] [-o <out.bed>] [-f]\n"
                    "                [--header] [--min-valid-coverage N] [--assign-code x:C] [--mask] [--missing quiet|warn|fail] [--device N] [--stats]\n"
                    "       mkpileup dmr sites -a <a.bed[.gz]> -b <b.bed[.gz]> --ref <ref.fa> --base C [--base A ..] [-o <out.bed>] [-f] [--header]\n"
                    "                [--min-valid-coverage N] [--assign-code x:C] [--mask] [--prior ALPHA BETA] [--delta D] [--max-coverages A B]\n"
                    "                [-N N] [--cap-coverages] [-i BP] [--batch-size N | -t T] [--device N] [--stats]\n"
                    "       mkpileup dmr replicates -a <a1.bed[.gz]> [-a <a2.bed[.gz]> ..] -b <b1.bed[.gz]> [-b ..] --ref <ref.fa> --base C [the flags of dmr sites]\n");
    return 2;
  }
  int rc = hemi ? mkp_pileup_hemi_main(argc - 2, (const char* const*)(argv + 2), err, sizeof(err)) : mkp_pileup_main(argc - 2,
      (const char* const*)(argv + 2), err, sizeof(err));
  if (rc != MKP_OK) { fprintf(stderr, "Error! %s (status %d)\n", err, rc); return 1; }
  return 0;
}
