// Stand-alone driver of the host tree stage of HDBSCAN (text_similarity_amd/csrc/hdbscan_tree.cpp) for a sanitizer build:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//         -Iinclude tests/hdbscan_tree_driver.cpp text_similarity_amd/csrc/hdbscan_tree.cpp -o driver
//     driver CASE_FILE
// tests/test_hdbscan_tree_sanitizer_cpu.py writes the case files and compares what this prints with the Python binding's
// results.  Every buffer handed to the library is a heap block of exactly the size the C ABI asks for, so that a byte read
// or written past it is a sanitizer report.
//
// Case file (little-endian): magic "HTC1", then int64 N, int32 min_cluster_size, int64 E (N - 1 in every well-formed call),
// E x int32 from, E x int32 to, E x float32 w2.
//
// Output: "rc RC", then for RC == 0 "clusters K" and "labels l0 l1 ...".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "tsim.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASE_FILE\n", argv[0]); return 2; }
    std::vector<char> buf;
    {
        std::ifstream f(argv[1], std::ios::binary);
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    if (buf.size() < 24 || memcmp(buf.data(), "HTC1", 4) != 0) { fprintf(stderr, "not a case file\n"); return 2; }
    int64_t N, E;
    int32_t mcs;
    memcpy(&N, buf.data() + 4, 8);
    memcpy(&mcs, buf.data() + 12, 4);
    memcpy(&E, buf.data() + 16, 8);
    if (E < 0 || N < -1 || N > (1 << 24) || buf.size() != 24 + (size_t)E * 12) { fprintf(stderr, "case file truncated\n"); return 2; }
    // the library reads N - 1 edges: the blocks hold exactly E of them and the test only writes cases with E == max(N - 1, 0)
    std::unique_ptr<int32_t[]> from(new int32_t[(size_t)E]), to(new int32_t[(size_t)E]);
    std::unique_ptr<float[]> w2(new float[(size_t)E]);
    memcpy(from.get(), buf.data() + 24, (size_t)E * 4);
    memcpy(to.get(), buf.data() + 24 + (size_t)E * 4, (size_t)E * 4);
    memcpy(w2.get(), buf.data() + 24 + (size_t)E * 8, (size_t)E * 4);
    std::unique_ptr<int32_t[]> labels(new int32_t[(size_t)(N > 0 ? N : 0)]);
    std::unique_ptr<int32_t> k(new int32_t(-7));
    const int rc = tsim_hdbscan_tree_labels(from.get(), to.get(), w2.get(), N, mcs, labels.get(), k.get());
    printf("rc %d\n", rc);
    if (rc == TSIM_OK) {
        printf("clusters %d\nlabels", (int)*k);
        for (int64_t i = 0; i < N; ++i) printf(" %d", (int)labels[i]);
        printf("\n");
    }
    return 0;
}
