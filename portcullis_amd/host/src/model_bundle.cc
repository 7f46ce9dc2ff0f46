// ModelBundle: see portcullis/ml/model_bundle.hpp.
#include <portcullis/ml/model_bundle.hpp>

#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>

namespace portcullis {
namespace ml {

namespace {
const char MAGIC[9] = "PJBMODL1";
const uint32_t ORDER = 5, PW_LEN = 32;
const char* const MODEL_NAMES[8] = {"exon", "intron", "donor_t", "donor_f", "acceptor_t", "acceptor_f", "donor_pw", "acceptor_pw"};
size_t rowsOf(size_t model) { return model < ModelBundle::KMER_MODELS ? ModelBundle::KMER_TABLE / 5 : ModelBundle::POS_TABLE / 5; }

void putU32(std::string& s, uint32_t v) {  // little-endian whatever the host is
    for (int k = 0; k < 4; k++) s.push_back((char)((v >> (8 * k)) & 0xff));
}
uint32_t getU32(const std::string& s, size_t at) {
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) v |= (uint32_t)(unsigned char)s[at + (size_t)k] << (8 * k);
    return v;
}
double getF64(const std::string& s, size_t at) {
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)(unsigned char)s[at + (size_t)k] << (8 * k);
    double d;
    memcpy(&d, &v, 8);
    return d;
}
}  // namespace

void ModelBundle::countSizes() {
    for (size_t m = 0; m < 8; m++) {
        const double* t = table(m);
        int32_t n = 0;
        for (size_t r = 0; r < rowsOf(m); r++) {
            bool any = false;
            for (int k = 0; k < 5; k++) any = any || t[r * 5 + (size_t)k] != 0.0;
            n += any;
        }
        sizes[m] = n;
    }
}

std::string ModelBundle::bytes() const {
    std::string s(MAGIC, 8);
    s.reserve(FILE_BYTES);
    putU32(s, L95);
    putU32(s, ORDER);
    putU32(s, PW_LEN);
    for (int k = 0; k < 8; k++) putU32(s, (uint32_t)sizes[k]);
    for (const double d : tables) {
        uint64_t v;
        memcpy(&v, &d, 8);
        for (int k = 0; k < 8; k++) s.push_back((char)((v >> (8 * k)) & 0xff));
    }
    return s;
}

void ModelBundle::save(const std::string& path) const {
    const std::string s = bytes();
    std::ofstream out(path.c_str(), std::ios::binary);
    out.write(s.data(), (std::streamsize)s.size());
    out.close();
    if (!out.good()) throw ModelBundleException("Could not write the Markov model file " + path);
}

std::string ModelBundle::check(const std::string& s) {
    std::ostringstream why;
    if (s.size() < 8 || memcmp(s.data(), MAGIC, 8) != 0) return "it does not start with the magic PJBMODL1 (not a Markov model file of portcullis_amd)";
    if (s.size() != FILE_BYTES) {
        why << "it is " << s.size() << " bytes long, a model file is " << FILE_BYTES << (s.size() < FILE_BYTES ? " (truncated)" : "");
        return why.str();
    }
    if (getU32(s, 12) != ORDER || getU32(s, 16) != PW_LEN) {
        why << "order " << getU32(s, 12) << " and " << getU32(s, 16) << " positions (this program scores with order " << ORDER << " and " << PW_LEN << " positions)";
        return why.str();
    }
    size_t at = 8 + 3 * 4 + 8 * 4;
    for (size_t m = 0; m < 8; m++) {
        int64_t trained = 0;
        for (size_t r = 0; r < rowsOf(m); r++) {
            double sum = 0.0;
            bool any = false;
            for (int k = 0; k < 5; k++, at += 8) {
                const double v = getF64(s, at);
                if (!std::isfinite(v) || v < 0.0 || v > 1.0) {
                    why << "model " << MODEL_NAMES[m] << ", row " << r << ", base " << k << " is " << v << ": not a probability";
                    return why.str();
                }
                sum += v;
                any = any || v != 0.0;
            }
            if (any && std::fabs(sum - 1.0) > 1e-12) {
                why.precision(17);
                why << "model " << MODEL_NAMES[m] << ", row " << r << " sums to " << sum << " (0 or 1 is expected)";
                return why.str();
            }
            trained += any;
        }
        const int32_t stated = (int32_t)getU32(s, 20 + 4 * m);
        if (stated != trained) {
            why << "model " << MODEL_NAMES[m] << " states " << stated << " trained rows and holds " << trained;
            return why.str();
        }
    }
    return "";
}

ModelBundle ModelBundle::load(const std::string& path) {
    std::ifstream in(path.c_str(), std::ios::binary);
    if (!in.good()) throw ModelBundleException("Could not open the Markov model file " + path);
    std::ostringstream buf;
    buf << in.rdbuf();
    const std::string s = buf.str();
    const std::string fault = check(s);
    if (!fault.empty()) throw ModelBundleException("The Markov model file " + path + " cannot be used: " + fault);
    ModelBundle b;
    b.L95 = getU32(s, 8);
    for (size_t k = 0; k < 8; k++) b.sizes[k] = (int32_t)getU32(s, 20 + 4 * k);
    for (size_t k = 0; k < TABLE_DOUBLES; k++) b.tables[k] = getF64(s, 52 + 8 * k);
    return b;
}

}  // namespace ml
}  // namespace portcullis
