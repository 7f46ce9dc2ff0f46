// Self-training's host side: see self_train.hpp.
#include "self_train.hpp"

#include <dirent.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "fs_util.hpp"
#include "rule_filter.hpp"

namespace portcullis {
namespace selftrain {

namespace {
// N of a name that ends in layerN.json (N: one digit or more), or -1
long layerNumber(const std::string& name) {
    const std::string tail = ".json";
    if (name.size() <= tail.size() || name.compare(name.size() - tail.size(), tail.size(), tail) != 0) return -1;
    size_t e = name.size() - tail.size(), b = e;
    while (b > 0 && name[b - 1] >= '0' && name[b - 1] <= '9') b--;
    if (b == e || e - b > 9 || b < 5 || name.compare(b - 5, 5, "layer") != 0) return -1;
    return std::strtol(name.substr(b, e - b).c_str(), nullptr, 10);
}
size_t count(const std::vector<char>& mask) { return (size_t)std::count(mask.begin(), mask.end(), (char)1); }
std::vector<size_t> indices(const std::vector<char>& mask) {
    std::vector<size_t> v;
    for (size_t r = 0; r < mask.size(); r++)
        if (mask[r]) v.push_back(r);
    return v;
}
}  // namespace

Layers findLayers(const std::string& trainingRule, const std::string& dataDir) {
    Layers l;
    l.ruleset = isDirectory(trainingRule) ? trainingRule : dataDir + "/" + trainingRule;
    DIR* d = isDirectory(l.ruleset) ? opendir(l.ruleset.c_str()) : nullptr;
    if (!d) throw SelfTrainException("Could not find suitable directory containing training rules for ruleset");
    std::vector<std::pair<long, std::string>> pos, neg;
    while (const dirent* e = readdir(d)) {
        const std::string name = e->d_name;
        const long n = layerNumber(name);
        if (n < 0) continue;
        if (name.find("neg") != std::string::npos) neg.emplace_back(n, l.ruleset + "/" + name);
        else if (name.find("pos") != std::string::npos) pos.emplace_back(n, l.ruleset + "/" + name);
    }
    closedir(d);
    if (pos.empty() || neg.empty()) throw SelfTrainException("Not enough positive and negative layers found in " + trainingRule + " ruleset.");
    std::sort(pos.begin(), pos.end());  // (by layer number; two files of one number: by name, where the reference leaves the order open)
    std::sort(neg.begin(), neg.end());
    for (const auto& p : pos) l.pos.push_back(p.second);
    for (const auto& p : neg) l.neg.push_back(p.second);
    return l;
}

TrainingSets createTrainingSets(const std::vector<std::string>& fieldnames, const std::vector<std::vector<std::string>>& rows,
                                const std::vector<std::string>& posLayerFiles, const std::vector<std::string>& negLayerFiles) {
    const size_t n = rows.size();
    auto column = [&](const char* name) {
        const auto it = std::find(fieldnames.begin(), fieldnames.end(), name);
        if (it == fieldnames.end()) throw SelfTrainException(std::string("The junction table has no column ") + name);
        const size_t at = (size_t)(it - fieldnames.begin());
        std::vector<double> v(n);
        for (size_t r = 0; r < n; r++) v[r] = std::strtod(rows[r].at(at).c_str(), nullptr);
        return v;
    };
    const std::vector<double> size = column("size"), maxmmes = column("maxmmes");
    // A rule is evaluated over the whole table -- a column is numeric or not by all of its values, as read_csv decided for the
    // script -- and a layer is the rows of its input that pass.
    auto passes = [&](const std::string& file) { return RuleFilter::load(file).evaluate(fieldnames, rows); };
    TrainingSets out;
    std::string& log = out.log;
    log += "LAYER\tPASS\tFAIL\n";
    std::vector<char> input(n, 1), pos(n, 1);
    size_t layer = 0;
    for (const std::string& file : posLayerFiles) {
        layer++;
        std::vector<char> in = passes(file);
        for (size_t r = 0; r < n; r++) in[r] = in[r] && input[r];
        log += std::to_string(layer) + "\t" + std::to_string(count(in)) + "\t" + std::to_string(n - count(in)) + "\n";
        out.posLayers.push_back(indices(in));
        if (count(in) <= 100) {  // the layer's input stands, and no further layer is applied
            log += "WARNING: We recommend at least 100 junctions in the positive set and this set of rules lowered the positive set to " +
                   std::to_string(count(in)) + " .  Will not filter positive set further.\n";
            pos = input;
            break;
        }
        pos = in;
        input = in;
    }
    if (count(pos) == 0) throw SelfTrainException("Can't build training sets, positive set filter left no junctions remaining.");
    std::vector<double> sizes;
    for (size_t r = 0; r < n; r++)
        if (pos[r]) sizes.push_back(size[r]);
    std::sort(sizes.begin(), sizes.end());
    out.L95 = (uint32_t)sizes[(size_t)((double)sizes.size() * 0.95)];
    const long posLimit = (long)((double)out.L95 * 1.2);
    log += "Intron size at L95 = " + std::to_string(out.L95) + "  positive set maximum intron size limit set to L95 x 1.2: " + std::to_string(posLimit) + "\n";
    if (count(pos) > 100) {
        for (size_t r = 0; r < n; r++) pos[r] = pos[r] && size[r] <= (double)posLimit;
        log += std::to_string(layer + 1) + "\t" + std::to_string(count(pos)) + "\t" + std::to_string(n - count(pos)) + "\n";
        out.posSizeLayer = true;
        out.posLayers.push_back(indices(pos));
    }
    out.pos = indices(pos);
    // the negative set: every layer takes its matches from what the layers before it left
    std::vector<char> other(n), neg(n, 0);
    for (size_t r = 0; r < n; r++) other[r] = !pos[r];
    log += std::to_string(count(other)) + " remaining for consideration as negative set\nLAYER\tPASS\tFAIL\n";
    layer = 0;
    for (const std::string& file : negLayerFiles) {
        layer++;
        const std::vector<char> hit = passes(file);
        std::vector<char> took(n, 0);
        for (size_t r = 0; r < n; r++) {
            took[r] = other[r] && hit[r];
            other[r] = other[r] && !hit[r];
            neg[r] = neg[r] || took[r];
        }
        log += std::to_string(layer) + "\t" + std::to_string(count(took)) + "\t" + std::to_string(count(other)) + "\n";
        out.negLayers.push_back(indices(took));
    }
    const long negLimit = (long)out.L95 * 8;
    std::vector<char> took(n, 0);
    for (size_t r = 0; r < n; r++) {
        took[r] = other[r] && size[r] > (double)negLimit && maxmmes[r] < 12.0;
        neg[r] = neg[r] || took[r];
    }
    log += "Intron size L95 = " + std::to_string(out.L95) + " negative set will use junctions with intron size over L95 x 8: " + std::to_string(negLimit) +
           " and with maxmmes < 12\n" + std::to_string(layer + 1) + "\t" + std::to_string(count(took)) + "\t" + std::to_string(count(other)) + "\n";
    out.negLayers.push_back(indices(took));
    out.neg = indices(neg);
    return out;
}

uint32_t uniformInt(std::mt19937& gen, uint32_t hi) {  // bits/uniform_int_dist.h: _S_nd<uint64_t> (Lemire's multiply-high with rejection)
    const uint32_t range = hi + 1;
    uint64_t product = (uint64_t)gen() * range;
    uint32_t low = (uint32_t)product;
    if (low < range) {
        const uint32_t threshold = (0u - range) % range;
        while (low < threshold) {
            product = (uint64_t)gen() * range;
            low = (uint32_t)product;
        }
    }
    return (uint32_t)(product >> 32);
}

double uniformReal(std::mt19937& gen) {  // bits/random.tcc: generate_canonical<double, 53> on a 32-bit generator: two draws, the low word first
    double sum = (double)gen();
    sum += (double)gen() * 4294967296.0;
    const double r = sum / 18446744073709551616.0;
    return r >= 1.0 ? std::nextafter(1.0, 0.0) : r;
}

std::vector<double> smoteSynthesize(const double* data, size_t rows, size_t cols, const uint32_t* nn, size_t k, uint32_t smoteness) {
    if (smoteness < 1) smoteness = 1;
    std::vector<double> synthetic(smoteness * rows * cols);
    std::mt19937 rng(SEED);
    size_t at = 0;
    for (size_t i = 0; i < rows; i++)
        for (uint32_t rep = 0; rep < smoteness; rep++) {
            const size_t j = nn[i * k + uniformInt(rng, (uint32_t)k - 1)];
            for (size_t c = 0; c < cols; c++) {
                const double dif = data[j * cols + c] - data[i * cols + c];
                const double gap = uniformReal(rng);
                const double step = gap * dif;  // (rounded on its own: the reference is built without contraction)
                synthetic[at++] = data[i * cols + c] + step;
            }
        }
    return synthetic;
}

std::vector<size_t> undersample(size_t size, size_t keep) {
    std::vector<size_t> left(size);
    for (size_t i = 0; i < size; i++) left[i] = i;
    std::mt19937 rng(SEED);
    while (left.size() > keep) {
        const size_t i = uniformInt(rng, (uint32_t)left.size());  // (inclusive: one past the last index can be drawn)
        if (i == left.size()) left.pop_back();
        else left.erase(left.begin() + (std::ptrdiff_t)i);
    }
    return left;
}

std::vector<char> ennKeep(const uint32_t* nn, size_t rows, size_t k, const std::vector<char>& labels, uint32_t threshold) {
    std::vector<char> keep(rows, 0);
    for (size_t i = 0; i < rows; i++) {
        uint32_t same = 0;
        for (size_t j = 0; j < k; j++) same += (labels[nn[i * k + j]] != 0) == (labels[i] != 0);
        keep[i] = same >= threshold;
    }
    return keep;
}

}  // namespace selftrain
}  // namespace portcullis
