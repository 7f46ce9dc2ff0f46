// ml::ModelBundle (portcullis/ml/model_bundle.hpp) on its own: save, load and check, and the faults check names.  Host code only; built
// with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_host_model_bundle.py.
//   model_bundle_check selftest <dir>        every case below; prints "ok <n> checks"
//   model_bundle_check make <out> <kind>     writes a bundle: kind = trained | untrained
//   model_bundle_check check <file>          prints "ok L95 <l95> sizes <8 sizes>" or the fault (exit status 3)
#include <portcullis/ml/model_bundle.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>

using portcullis::ml::ModelBundle;
using portcullis::ml::ModelBundleException;

static int g_checks = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        g_checks++;                                                       \
        if (!(cond)) {                                                    \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

// a bundle as a training leaves it: in every model some rows trained, each of them count / sum of small integers
static ModelBundle trained() {
    ModelBundle b;
    b.L95 = 4321;
    for (size_t m = 0; m < 8; m++) {
        const size_t rows = m < ModelBundle::KMER_MODELS ? ModelBundle::KMER_TABLE / 5 : ModelBundle::POS_TABLE / 5;
        for (size_t r = m % 3; r < rows; r += 3 + m) {
            unsigned cnt[5], sum = 0;
            for (int k = 0; k < 5; k++) sum += cnt[k] = (unsigned)((r * 7 + m * 13 + (size_t)k * 5) % 11);
            if (!sum) sum = cnt[2] = 3;
            for (int k = 0; k < 5; k++) b.table(m)[r * 5 + (size_t)k] = (double)cnt[k] / (double)sum;
        }
    }
    b.countSizes();
    return b;
}

static void putF64(std::string& s, size_t at, double d) {
    unsigned long long v;
    memcpy(&v, &d, 8);
    for (int k = 0; k < 8; k++) s[at + (size_t)k] = (char)((v >> (8 * k)) & 0xff);
}
static bool names(const std::string& fault, const char* what) { return fault.find(what) != std::string::npos; }

static int selftest(const std::string& dir) {
    const size_t TABLES_AT = 8 + 3 * 4 + 8 * 4;
    const ModelBundle t = trained(), u;
    EXPECT(t.bytes().size() == ModelBundle::FILE_BYTES && ModelBundle::FILE_BYTES == 752612);
    EXPECT(ModelBundle::check(t.bytes()).empty());
    EXPECT(ModelBundle::check(u.bytes()).empty());  // the untrained, all-zero one
    for (int k = 0; k < 8; k++) EXPECT(u.sizes[k] == 0 && t.sizes[k] > 0);
    // save -> load -> the same bytes
    for (const ModelBundle* b : {&t, &u}) {
        const std::string path = dir + (b == &t ? "/trained.models" : "/untrained.models");
        b->save(path);
        const ModelBundle back = ModelBundle::load(path);
        EXPECT(back.L95 == b->L95 && back.tables == b->tables && memcmp(back.sizes, b->sizes, sizeof back.sizes) == 0);
        EXPECT(back.bytes() == b->bytes());
    }
    // the little-endian layout, byte by byte
    const std::string s = t.bytes();
    EXPECT(s.compare(0, 8, "PJBMODL1") == 0);
    EXPECT((unsigned char)s[8] == (4321 & 0xff) && (unsigned char)s[9] == (4321 >> 8) && s[10] == 0 && s[11] == 0);
    EXPECT(s[12] == 5 && s[16] == 32);
    EXPECT((unsigned char)s[20] == (unsigned)(t.sizes[0] & 0xff));
    // faults
    std::string x = s;
    x[0] = 'Q';
    EXPECT(names(ModelBundle::check(x), "magic"));
    EXPECT(names(ModelBundle::check(s.substr(0, s.size() - 1)), "truncated") && names(ModelBundle::check(s + "x"), "bytes long"));
    EXPECT(names(ModelBundle::check(std::string()), "magic") && names(ModelBundle::check("PJBMODL1"), "truncated"));
    x = s;
    x[12] = 4;
    EXPECT(names(ModelBundle::check(x), "order 4"));
    x = s;
    x[16] = 24;
    EXPECT(names(ModelBundle::check(x), "24 positions"));
    size_t row = 0;  // a trained row of the exon model
    while (t.table(0)[row * 5] == 0.0 && t.table(0)[row * 5 + 1] == 0.0 && t.table(0)[row * 5 + 2] == 0.0) row++;
    for (const double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -0.25, 1.5}) {
        x = s;
        putF64(x, TABLES_AT + row * 40, bad);
        EXPECT(names(ModelBundle::check(x), "not a probability") && names(ModelBundle::check(x), "exon"));
    }
    x = s;  // a row summing to 0.5
    for (int k = 0; k < 5; k++) putF64(x, TABLES_AT + row * 40 + 8 * (size_t)k, k < 2 ? 0.25 : 0.0);
    EXPECT(names(ModelBundle::check(x), "sums to 0.5"));
    x = s;  // a wrong size
    x[20 + 4 * 7] = (char)(x[20 + 4 * 7] + 1);
    EXPECT(names(ModelBundle::check(x), "acceptor_pw states"));
    x = s;  // a row zeroed without the size following
    for (int k = 0; k < 5; k++) putF64(x, TABLES_AT + row * 40 + 8 * (size_t)k, 0.0);
    EXPECT(names(ModelBundle::check(x), "exon states"));
    // load names the file and the fault; a file that is not there is said to be so
    {
        std::ofstream out((dir + "/bad.models").c_str(), std::ios::binary);
        out << s.substr(0, 1000);
    }
    try {
        (void)ModelBundle::load(dir + "/bad.models");
        EXPECT(false);
    } catch (const ModelBundleException& e) {
        EXPECT(names(e.what(), "bad.models") && names(e.what(), "truncated"));
    }
    try {
        (void)ModelBundle::load(dir + "/nosuch.models");
        EXPECT(false);
    } catch (const ModelBundleException& e) {
        EXPECT(names(e.what(), "nosuch.models"));
    }
    printf("ok %d checks\n", g_checks);
    return 0;
}

int main(int argc, char* argv[]) {
    try {
        if (argc == 3 && !strcmp(argv[1], "selftest")) return selftest(argv[2]);
        if (argc == 4 && !strcmp(argv[1], "make")) {
            (strcmp(argv[3], "trained") == 0 ? trained() : ModelBundle()).save(argv[2]);
            return 0;
        }
        if (argc == 3 && !strcmp(argv[1], "check")) {
            const ModelBundle b = ModelBundle::load(argv[2]);
            printf("ok L95 %u sizes", b.L95);
            for (int k = 0; k < 8; k++) printf(" %d", b.sizes[k]);
            printf("\n");
            return 0;
        }
    } catch (const ModelBundleException& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    fprintf(stderr, "usage: model_bundle_check selftest <dir> | make <out> trained|untrained | check <file>\n");
    return 2;
}
