// bioinfo1_amd/csrc/tm_main.cpp -- team_mapper_amd: the reference mapper's
// command line (team_mapper.cpp:165-180, 319-396) over the MI355X pipeline
// (tm_map_files).  PAF-like lines go to stdout in read order.
#include <cerrno>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/team_align_c.h"
#include "../../include/team_mapper_c.h"

#define TM_VERSION "3.1.0"
#define TM_PROGRAM "toolForGenomeAllignment"

static void help() {
    std::printf(
        "\nUsage: %s[options] <file1> <file2>\n"
        "NOTE: file1 needs to be in FASTA format, while the second file will contain a set of fragments in either "
        "FASTA or FASTQ format.\n"
        "Options: \n"
        "\t  -a, --alignment TYPE     Alignment type: global, local, semiGlobal\n"
        "\t  -m MATCH                 Match score (default: 1)\n"
        "\t  -n MISMATCH              Mismatch penalty (default: -1)\n"
        "\t  -g GAP                   Gap penalty (default: -1)\n"
        "\t  -k KMER                  k-mer length for minimizers (default: 15)\n"
        "\t  -w WINDOW                window size for minimizers (default: 5)\n"
        "\t  -f FREQUENCY_THRESHOLD   Frequency threshold factor (default: 0.001)\n"
        "\t  -c                       Output CIGAR string\n"
        "\t  -h, --help               Show this help message\n"
        "\t  --version                Show version information\n"
        "\t  -d DEVICE                GPU index (default: 0)\n",
        TM_PROGRAM);
}

int main(int argc, char** argv) {
    tm_options o{TA_GLOBAL, 1, -1, -1, 15, 5, 0.001, 0, 0};
    std::string f1, f2;
    int device = 0;
    unsigned flags = 0;  // --eqx: =/X CIGARs and an NM tag (not in help(), which restates the reference's text)
    bool banded = false;  // --band N: every window through the banded extension (not in help() either)
    unsigned band = 0;
    bool band_auto = false;  // --band auto: a certified band per window, the unbanded results (not in help() either)
    bool affine = false;  // --gap-open O (with --band): affine gaps, -g is the gap extend (not in help() either)
    int gap_open = 0;
    bool extend_ends = false;  // --extend-ends (with --band N, -a global): windows extended to the read's ends (not in help())
    int zdrop = -1;  // --zdrop Z (with --extend-ends): both end extensions stop once the end has died (not in help())
    bool zdrop_rule_given = false;  // --zdrop-rule segment|stripe (with --zdrop): which rule decides the drop (not in help())
    int zdrop_rule = TA_ZDROP_SEGMENT;
    if (argc < 2) {
        std::fprintf(stderr, "Error: Not enough arguments\n");
        help();
        return 1;
    }
    if (!std::strcmp(argv[1], "-h") || !std::strcmp(argv[1], "--help")) {
        help();
        return 0;
    }
    if (!std::strcmp(argv[1], "--version")) {
        std::printf("%s v%s\n", TM_PROGRAM, TM_VERSION);
        return 0;
    }
    if (argc < 3) {
        std::fprintf(stderr, "Error: Expected two input files\n");
        return 1;
    }
    for (int i = 1; i < argc; ++i) {
        const char* a = argv[i];
        const bool more = i + 1 < argc;
        if (!std::strcmp(a, "-a") && more) {
            const char* t = argv[++i];
            if (!std::strcmp(t, "global")) o.type = TA_GLOBAL;
            else if (!std::strcmp(t, "local")) o.type = TA_LOCAL;
            else if (!std::strcmp(t, "semiGlobal")) o.type = TA_SEMI_GLOBAL;
            else {
                std::fprintf(stderr, "Error: Expected Alignment type: global, local, semiGlobal\n");
                help();
                return 1;
            }
        } else if (!std::strcmp(a, "-m") && more) o.match = std::atoi(argv[++i]);
        else if (!std::strcmp(a, "-n") && more) o.mismatch = std::atoi(argv[++i]);
        else if (!std::strcmp(a, "-g") && more) o.gap = std::atoi(argv[++i]);
        else if (!std::strcmp(a, "-k") && more) o.k = (unsigned)std::atoi(argv[++i]);
        else if (!std::strcmp(a, "-w") && more) o.w = (unsigned)std::atoi(argv[++i]);
        else if (!std::strcmp(a, "-f") && more) o.f = std::strtod(argv[++i], nullptr);
        else if (!std::strcmp(a, "-d") && more) device = std::atoi(argv[++i]);
        else if (!std::strcmp(a, "-c")) o.want_cigar = 1;
        else if (!std::strcmp(a, "--eqx")) flags |= TM_MAP_EQX;
        else if (!std::strcmp(a, "--extend-ends")) extend_ends = true;
        else if (!std::strcmp(a, "--band") && more && !std::strcmp(argv[i + 1], "auto")) {
            ++i;
            banded = band_auto = true;
        }
        else if (!std::strcmp(a, "--band") && more) {
            char* end = nullptr;
            const unsigned long long v = std::strtoull(argv[++i], &end, 10);
            if (end == argv[i] || *end || argv[i][0] == '-' || v > 0xFFFFFFFFull) {
                std::fprintf(stderr, "Error: --band expects a number in [0, 2^32)\n");
                return 1;
            }
            banded = true;
            band_auto = false;
            band = (unsigned)v;
        }
        else if (!std::strcmp(a, "--gap-open") && more) {
            char* end = nullptr;
            errno = 0;
            const long v = std::strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end || errno || v < INT_MIN || v > INT_MAX) {
                std::fprintf(stderr, "Error: --gap-open expects a decimal integer\n");
                return 1;
            }
            affine = true;
            gap_open = (int)v;
        }
        else if (!std::strcmp(a, "--zdrop") && more) {
            char* end = nullptr;
            errno = 0;
            const long v = std::strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end || errno || argv[i][0] == '-' || argv[i][0] == '+' || v < 0 || v > INT_MAX) {
                std::fprintf(stderr, "Error: --zdrop expects a decimal integer in [0, 2^31)\n");
                return 1;
            }
            zdrop = (int)v;
        }
        else if (!std::strcmp(a, "--zdrop-rule") && more) {
            const char* v = argv[++i];
            if (!std::strcmp(v, "segment")) zdrop_rule = TA_ZDROP_SEGMENT;
            else if (!std::strcmp(v, "stripe")) zdrop_rule = TA_ZDROP_STRIPE;
            else {
                std::fprintf(stderr, "Error: --zdrop-rule expects segment or stripe\n");
                return 1;
            }
            zdrop_rule_given = true;
        }
        else if (!std::strcmp(a, "-s")) std::fprintf(stderr, "note: -s (statistics) is not part of this build\n");
        else if (f1.empty()) f1 = a;
        else if (f2.empty()) f2 = a;
        else {
            std::fprintf(stderr, "Unknown or extra argument: %s\n", a);
            help();
            return 1;
        }
    }
    if (f1.empty() || f2.empty()) {
        std::fprintf(stderr, "Error: Two input files are required.\n");
        help();
        return 1;
    }
    if (affine && !banded) {
        std::fprintf(stderr, "Error: --gap-open requires --band (there is no unbanded affine mapper path)\n");
        return 1;
    }
    if (extend_ends) {
        const char* why = band_auto ? "a numeric --band, not --band auto"
                          : !banded ? "--band N"
                          : o.type != TA_GLOBAL ? "-a global"
                          : (flags & TM_MAP_EQX) ? "a run without --eqx"
                                                 : nullptr;
        if (why) {
            std::fprintf(stderr, "Error: --extend-ends requires %s\n", why);
            return 1;
        }
    }
    if (zdrop >= 0 && !extend_ends) {
        std::fprintf(stderr, "Error: --zdrop requires --extend-ends\n");
        return 1;
    }
    if (zdrop_rule_given && zdrop < 0) {
        std::fprintf(stderr, "Error: --zdrop-rule requires --zdrop\n");
        return 1;
    }
    // (the band caveat: the segment rule follows the fill's step order; the stripe rule, §3.20, does not)
    if (zdrop >= 0 && band > 32 && zdrop_rule == TA_ZDROP_SEGMENT)
        std::fprintf(stderr, "warning: --zdrop with --band above 32 can clip a live end longer than 1024 bases at "
                             "row 1024; use --band 32 or less, or a large Z\n");
    const int r = extend_ends ? tm_map_files_band_ends_zdrop_rule(f1.c_str(), f2.c_str(), &o, "-", device, flags, band,
                                                                  affine ? &gap_open : nullptr, zdrop, zdrop_rule)
                  : band_auto ? tm_map_files_band_exact(f1.c_str(), f2.c_str(), &o, "-", device, flags,
                                                      affine ? &gap_open : nullptr)
                  : affine   ? tm_map_files_band_affine(f1.c_str(), f2.c_str(), &o, "-", device, flags, band, gap_open)
                  : banded ? tm_map_files_band(f1.c_str(), f2.c_str(), &o, "-", device, flags, band)
                           : tm_map_files_x(f1.c_str(), f2.c_str(), &o, "-", device, flags);
    if (r != TM_OK && r != TM_ERR_INPUT) std::fprintf(stderr, "error: %s\n", tm_status_string(r));
    return r == TM_OK ? 0 : 1;
}
