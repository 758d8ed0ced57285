// gzip_trial.cpp -- TEST-ONLY: the host's walk of the gzip kernels (rsq_deflate.h: gzip_on_the_host) over a file of texts, a program of its own so that it can be built
// with -fsanitize=address,undefined and run as it is (tests/test_device_gzip.py builds it with g++ and runs it).  Every text goes by both routes through the walk that
// reads the text where it lies and through the walk that reads it through a ring like the kernel's (RingPiece: the ring's index arithmetic, the bytes behind a piece's
// end); the two must write the same members.
// The file: per text a 64-bit length (little endian) and the bytes.  Exit status 0: all equal; 1: a difference (named on stderr); 2: usage or a file that cannot be read.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_deflate.h"

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: gzip_trial FILE_OF_TEXTS\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "gzip_trial: cannot open %s\n", argv[1]);
        return 2;
    }
    int bad = 0;
    size_t n_texts = 0, n_bytes = 0;
    uint64_t len;
    while (fread(&len, 8, 1, f) == 1) {
        // an allocation of exactly the text's size: a read behind its end is a read behind the allocation
        std::vector<uint8_t> text((size_t)len);
        if (len && fread(text.data(), 1, (size_t)len, f) != len) {
            fprintf(stderr, "gzip_trial: text %zu is cut short\n", n_texts);
            fclose(f);
            return 2;
        }
        for (int route = 0; route < 2; ++route) {
            std::vector<uint8_t> plain, ring;
            rsq::gz::gzip_on_the_host(text.data(), len, plain, route, -1);
            rsq::gz::gzip_on_the_host(text.data(), len, ring, route, 'I');
            if (plain != ring) {
                fprintf(stderr, "gzip_trial: text %zu (%llu bytes), route %d: the walk through the ring writes other members (%zu bytes) than the walk over the text (%zu bytes)\n", n_texts,
                        (unsigned long long)len, route, ring.size(), plain.size());
                bad = 1;
            }
            n_bytes += plain.size();
        }
        ++n_texts;
    }
    fclose(f);
    printf("gzip_trial: %zu texts by two routes, %zu bytes of members\n", n_texts, n_bytes);
    return bad;
}
