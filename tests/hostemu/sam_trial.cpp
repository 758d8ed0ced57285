// sam_trial.cpp -- TEST-ONLY: truth_trial.h for SAM text; the records lie at the start of `sam`, segment 0 first
#include "truth_trial.h"

extern "C" int sam_trial(const truth_trial_pair *in, char *fastq0, char *fastq1, char *sam, uint32_t cap, uint32_t *sizes) {
    return truth_trial<SamFormat>(in, fastq0, fastq1, sam, 0u, cap, sizes);
}
