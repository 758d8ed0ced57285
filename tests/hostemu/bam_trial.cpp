// bam_trial.cpp -- TEST-ONLY: truth_trial.h for BAM records; they lie at bam + at, segment 0 first
#include "truth_trial.h"

extern "C" int bam_trial(const truth_trial_pair *in, char *fastq0, char *fastq1, char *bam, uint32_t at, uint32_t cap, uint32_t *sizes) {
    return truth_trial<BamFormat>(in, fastq0, fastq1, bam, at, cap, sizes);
}
