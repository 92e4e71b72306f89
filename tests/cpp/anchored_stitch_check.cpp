// tests/cpp/anchored_stitch_check.cpp -- the mapper's host stitcher
// (bioinfo1_amd/csrc/tm_stitch.h) as a program of its own, built with g++
// -fsanitize=address,undefined (tests/test_anchored_ref.py).  Reads lines
// "left|mid|right" from stdin, the empty op string written "1_" (for "1\0"),
// and prints one stitched CIGAR per line in the same spelling; "!" for a
// malformed piece.
#include <cstdio>
#include <iostream>
#include <string>

#include "tm_stitch.h"

static std::string piece(const std::string& s) { return s == "1_" ? std::string("1\0", 2) : s; }

int main() {
    std::string line, out;
    while (std::getline(std::cin, line)) {
        const size_t a = line.find('|'), b = line.find('|', a == std::string::npos ? a : a + 1);
        if (a == std::string::npos || b == std::string::npos) {
            std::puts("!");
            continue;
        }
        // exact-size heap copies, so that a read past a piece's end is an ASan error
        const std::string l = piece(line.substr(0, a)), m = piece(line.substr(a + 1, b - a - 1)),
                          r = piece(line.substr(b + 1));
        char* lb = new char[l.size() + 1];
        char* mb = new char[m.size() + 1];
        char* rb = new char[r.size() + 1];
        l.copy(lb, l.size());
        m.copy(mb, m.size());
        r.copy(rb, r.size());
        const bool ok = tmap::stitch_cigar(lb, l.size(), mb, m.size(), rb, r.size(), out);
        delete[] lb;
        delete[] mb;
        delete[] rb;
        if (!ok) std::puts("!");
        else if (out == std::string("1\0", 2)) std::puts("1_");
        else std::puts(out.c_str());
    }
    return 0;
}
