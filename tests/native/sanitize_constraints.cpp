// sanitize_constraints.cpp -- the loader of the constraints file (bisbm_io_read_constraints, csrc/bisbm_io.cpp: the scanner and the
// turning of the lists into classes) under AddressSanitizer + UndefinedBehaviorSanitizer.  A program of its own: it is compiled
// with the sanitizers together with bisbm_io.cpp and run as it is (tests/test_constraints.py).  Every input is written to a file in
// the directory given as argv[1] and loaded for a graph of 6 + 4 nodes and 3 + 2 blocks; the good ones are checked cell by cell,
// the malformed ones must be refused with the offending token in the message and both outputs NULL.  Exit 0: all as stated.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bisbm_io.h"

namespace {

int failures = 0;

#define EXPECT(cond, what)                                                       \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, (what)); \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

const uint64_t N = 10, NA = 6;
const uint32_t KA = 3, KB = 2, K = 5;

std::string write(const std::string& dir, const std::string& text) {
    const std::string path = dir + "/constraints.txt";
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) std::exit(2);
    std::fwrite(text.data(), 1, text.size(), f);
    std::fclose(f);
    return path;
}

void refused(const std::string& dir, const std::string& text, const std::string& token) {
    uint8_t *cls = (uint8_t*)1, *allowed = (uint8_t*)1;
    char err[512];
    const long rc = bisbm_io_read_constraints(write(dir, text).c_str(), N, NA, KA, KB, &cls, &allowed, err, sizeof(err));
    EXPECT(rc == -2, text.c_str());
    EXPECT(cls == nullptr && allowed == nullptr, text.c_str());
    EXPECT(std::strstr(err, ("'" + token + "'").c_str()) != nullptr, err);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    char err[512];
    uint8_t *cls = nullptr, *allowed = nullptr;

    // any order, blanks and tabs, a carriage return, a repeat with the same blocks in another order, no line end at the end
    long rc = bisbm_io_read_constraints(write(dir, "7 4\n\n 0 1\t0 \r\n3  2\n0 0 1\n9 4").c_str(), N, NA, KA, KB, &cls, &allowed, err, sizeof(err));
    EXPECT(rc == 4, err);
    if (rc == 4) {
        const uint8_t want_cls[10] = {2, 0, 0, 3, 0, 0, 0, 1, 0, 1};
        const uint8_t want[4][5] = {{1, 1, 1, 1, 1}, {1, 1, 1, 0, 1}, {1, 1, 0, 1, 1}, {0, 0, 1, 1, 1}};
        EXPECT(std::memcmp(cls, want_cls, 10) == 0, "classes");
        EXPECT(std::memcmp(allowed, want, 20) == 0, "table");
    }
    bisbm_io_free(cls);
    bisbm_io_free(allowed);

    // an empty file, and one of blank lines: class 0 alone
    for (const char* text : {"", "\n", "  \n\t\r\n"}) {
        rc = bisbm_io_read_constraints(write(dir, text).c_str(), N, NA, KA, KB, &cls, &allowed, err, sizeof(err));
        EXPECT(rc == 1, err);
        if (rc == 1) {
            for (uint64_t v = 0; v < N; ++v) EXPECT(cls[v] == 0, "class 0");
            for (uint32_t s = 0; s < K; ++s) EXPECT(allowed[s] == 1, "all allowed");
        }
        bisbm_io_free(cls);
        bisbm_io_free(allowed);
    }
    // NULL outputs and a NULL message buffer are allowed
    EXPECT(bisbm_io_read_constraints(write(dir, "1 0 2\n").c_str(), N, NA, KA, KB, nullptr, nullptr, nullptr, 0) == 2, "NULL outputs");
    EXPECT(bisbm_io_read_constraints(write(dir, "1 x\n").c_str(), N, NA, KA, KB, nullptr, nullptr, nullptr, 0) == -2, "NULL outputs");
    EXPECT(bisbm_io_read_constraints((dir + "/none.txt").c_str(), N, NA, KA, KB, &cls, &allowed, err, sizeof(err)) == -1, "no file");
    // a one-byte message buffer
    char tiny[1];
    EXPECT(bisbm_io_read_constraints(write(dir, "99 0\n").c_str(), N, NA, KA, KB, &cls, &allowed, tiny, sizeof(tiny)) == -2 && tiny[0] == 0, "tiny");

    refused(dir, "1 0\n10 3\n", "10");                          // an id >= n
    refused(dir, "1 0\n2 5\n", "5");                            // a block >= K
    refused(dir, "1 0\n2 3\n", "3");                            // a type-b block for a type-a node
    refused(dir, "7 1\n", "1");                                 // a type-a block for a type-b node
    refused(dir, "1 0\nx2 1\n", "x2");                          // a letter in the id
    refused(dir, "1 0\n2 1a\n", "1a");                          // ... in a block
    refused(dir, "1 -0\n", "-0");                               // a sign
    refused(dir, "1 0.5\n", "0.5");
    refused(dir, "18446744073709551616 0\n", "18446744073709551616");  // 2^64
    refused(dir, "1 99999999999999999999999\n", "99999999999999999999999");
    refused(dir, "1 0\n1 1\n", "1");                            // a node repeated with other blocks
    refused(dir, "4\n", "4");                                   // a node without a block
    refused(dir, std::string(300, '7') + " 0\n", std::string(300, '7'));  // a token longer than the message buffer's half

    // 255 distinct lists beside class 0 are taken, the 256th is refused: 300 nodes, 9 type-a blocks, node v lists the set bits of v + 1
    {
        const uint64_t n = 300;
        const uint32_t ka = 9;
        for (int lists : {255, 256}) {
            std::string text;
            for (int v = 0; v < lists; ++v) {
                text += std::to_string(v);
                for (uint32_t b = 0; b < ka; ++b)
                    if (((unsigned)(v + 1) >> b) & 1u) text += " " + std::to_string(b);
                text += "\n";
            }
            rc = bisbm_io_read_constraints(write(dir, text).c_str(), n, n, ka, 1, &cls, &allowed, err, sizeof(err));
            if (lists == 255) {
                EXPECT(rc == 256, err);
                if (rc == 256) EXPECT(cls[254] == 255 && cls[255] == 0 && allowed[255 * 10 + 9] == 1, "the last class");
            } else {
                EXPECT(rc == -2 && std::strstr(err, "'255'") != nullptr, err);
            }
            bisbm_io_free(cls);
            bisbm_io_free(allowed);
        }
    }
    if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
