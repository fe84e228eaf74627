// Stand-alone driver of the host tokenizer (text_similarity_amd/csrc/wordpiece.cpp) for a sanitizer build:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread
//         -Iinclude tests/wordpiece_driver.cpp text_similarity_amd/csrc/wordpiece.cpp -o driver
//     driver CASE_FILE
// tests/test_wordpiece_sanitizer_cpu.py writes the case files and compares what this prints with the Python binding's
// results.  Every buffer handed to the library is a heap block of exactly the size the C ABI asks for, so that a byte read
// or written past it is a sanitizer report.
//
// Case file (little-endian): magic "WPC1", then
//     int32 lowercase, max_chars, unk_id, max_len, n_threads, exact_capacity
//     blob  continuing prefix
//     int32 n_prefix, n_prefix x int32;  int32 n_suffix, n_suffix x int32
//     int32 n_vocab, n_vocab x blob;  int32 n_added, n_added x blob;  int64 n_sentences, n_sentences x blob
// where blob = int32 byte count + bytes.  exact_capacity != 0: out_capacity = bytes + n * specials, the least the ABI accepts
// for any max_len; otherwise bytes + n * max(specials, 1), what the Python binding allocates.
//
// Output: "create RC", "encode RC", then per sentence "i LEN HANDLED: id id ...".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "tsim.h"

namespace {

struct Reader {
    std::vector<char> buf;
    size_t at = 0;
    void need(size_t n) {
        if (n > buf.size() - at) { fprintf(stderr, "case file truncated at byte %zu\n", at); exit(2); }
    }
    int32_t i32() { need(4); int32_t v; memcpy(&v, buf.data() + at, 4); at += 4; return v; }
    int64_t i64() { need(8); int64_t v; memcpy(&v, buf.data() + at, 8); at += 8; return v; }
    std::string blob() {
        const int32_t n = i32();
        if (n < 0) { fprintf(stderr, "negative blob length at byte %zu\n", at); exit(2); }
        need((size_t)n);
        std::string s(buf.data() + at, (size_t)n);
        at += (size_t)n;
        return s;
    }
};

// strings back to back in a heap block of exactly their total size (no terminator), offsets in a block of n + 1
struct Packed {
    std::unique_ptr<char[]> text;
    std::unique_ptr<int64_t[]> off;
    int64_t bytes = 0;
    explicit Packed(const std::vector<std::string> &v) : off(new int64_t[v.size() + 1]) {
        off[0] = 0;
        for (size_t i = 0; i < v.size(); ++i) off[i + 1] = off[i] + (int64_t)v[i].size();
        bytes = off[v.size()];
        text.reset(new char[(size_t)bytes]);
        for (size_t i = 0; i < v.size(); ++i) memcpy(text.get() + off[i], v[i].data(), v[i].size());
    }
};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASE_FILE\n", argv[0]); return 2; }
    Reader r;
    {
        std::ifstream f(argv[1], std::ios::binary);
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        r.buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    r.need(4);
    if (memcmp(r.buf.data(), "WPC1", 4) != 0) { fprintf(stderr, "not a case file\n"); return 2; }
    r.at = 4;
    const int32_t lowercase = r.i32(), max_chars = r.i32(), unk_id = r.i32(), max_len = r.i32(), n_threads = r.i32(),
                  exact = r.i32();
    const std::string prefix = r.blob();
    std::vector<int32_t> pre((size_t)r.i32());
    for (auto &t : pre) t = r.i32();
    std::vector<int32_t> suf((size_t)r.i32());
    for (auto &t : suf) t = r.i32();
    std::vector<std::string> vocab((size_t)r.i32());
    for (auto &s : vocab) s = r.blob();
    std::vector<std::string> added((size_t)r.i32());
    for (auto &s : added) s = r.blob();
    std::vector<std::string> docs((size_t)r.i64());
    for (auto &s : docs) s = r.blob();

    void *h = nullptr;
    {
        Packed v(vocab), a(added);   // freed before encode: the handle must own what it keeps
        const int rc = tsim_wordpiece_create(v.text.get(), v.off.get(), (int32_t)vocab.size(), prefix.c_str(), unk_id,
                                             pre.empty() ? nullptr : pre.data(), (int32_t)pre.size(),
                                             suf.empty() ? nullptr : suf.data(), (int32_t)suf.size(), lowercase, max_chars,
                                             a.text.get(), a.off.get(), (int32_t)added.size(), &h);
        printf("create %d\n", rc);
        if (rc != TSIM_OK) return 1;
    }
    const int64_t n = (int64_t)docs.size();
    const int64_t nspec = (int64_t)(pre.size() + suf.size());
    Packed t(docs);
    const int64_t cap = t.bytes + n * (exact ? nspec : std::max<int64_t>(nspec, 1));
    std::unique_ptr<int32_t[]> ids(new int32_t[(size_t)cap]);
    std::unique_ptr<int32_t[]> lens(new int32_t[(size_t)n]);
    std::unique_ptr<uint8_t[]> handled(new uint8_t[(size_t)n]);
    const int rc = tsim_wordpiece_encode(h, t.text.get(), t.off.get(), n, max_len, n_threads, ids.get(), cap, lens.get(),
                                         handled.get());
    printf("encode %d\n", rc);
    if (rc == TSIM_OK) {
        int64_t o = 0;
        for (int64_t i = 0; i < n; ++i) {
            printf("%lld %d %d:", (long long)i, (int)lens[i], (int)handled[i]);
            for (int32_t k = 0; k < lens[i]; ++k) printf(" %d", (int)ids[o + k]);
            printf("\n");
            o += lens[i];
        }
    }
    tsim_wordpiece_destroy(h);
    return rc == TSIM_OK ? 0 : 1;
}
