// Performance / PerformanceList: the confusion matrix of one cross-validation fold and the table `train --folds` prints from the
// folds (lib/include/portcullis/ml/performance.hpp, lib/src/performance.cc of the reference).  Every rate is a percentage and is 0
// where its denominator is 0.  One deviation: where the reference's arithmetic leaves a NaN -- F1 with
// precision + recall = 0, MCC with informedness * markedness below 0 -- or the square root of -0.0, the value is 0, as the reference's
// own Python Performance has it; a NaN would poison the means.
#pragma once

#include <cstdint>
#include <memory>
#include <ostream>
#include <string>
#include <vector>

namespace portcullis {
namespace ml {

class Performance {
    uint32_t tp, tn, fp, fn;
    static double pct(uint32_t part, uint32_t whole) { return whole == 0 ? 0.0 : 100.0 * (double)part / (double)whole; }

public:
    Performance(uint32_t tp, uint32_t tn, uint32_t fp, uint32_t fn) : tp(tp), tn(tn), fp(fp), fn(fn) {}

    uint32_t getAllPositive() const { return tp + fp; }
    uint32_t getAllNegative() const { return tn + fn; }
    uint32_t getAllTrue() const { return tn + tp; }
    uint32_t getAllFalse() const { return fn + fp; }
    uint32_t getRealPositive() const { return tp + fn; }
    uint32_t getRealNegative() const { return fp + tn; }
    uint32_t getAll() const { return tp + tn + fp + fn; }

    double getPrecision() const { return pct(tp, getAllPositive()); }
    double getRecall() const { return pct(tp, getRealPositive()); }
    double getSensitivity() const { return getRecall(); }
    double getSpecificity() const { return pct(tn, getRealNegative()); }
    double getNPV() const { return pct(tn, getAllNegative()); }
    double getPrevalence() const { return pct(getRealPositive(), getAll()); }
    double getBias() const { return pct(getAllPositive(), getAll()); }
    double getAccuracy() const { return pct(getAllTrue(), getAll()); }
    double getInformedness() const { return getSensitivity() + getSpecificity() - 100.0; }
    double getMarkedness() const { return getPrecision() + getNPV() - 100.0; }
    double getFBScore(double beta) const;
    double getF1Score() const { return getFBScore(1.0); }
    double getMCC() const;

    // TP TN FP FN as integers, then PREV BIAS SENS SPEC PPV NPV F1 ACC INFO MARK MCC with two decimals, tab-joined
    std::string toLongString() const;
    static std::string longHeader() { return "TP\tTN\tFP\tFN\tPREV\tBIAS\tSENS\tSPEC\tPPV\tNPV\tF1\tACC\tINFO\tMARK\tMCC"; }
    static std::string to_2dp_string(double v);
};

class PerformanceList {
    std::vector<std::shared_ptr<Performance>> scores;
    static void outputMeanScore(const std::vector<double>& values, const std::string& name, std::ostream& out);

public:
    void clear() { scores.clear(); }
    size_t size() const { return scores.size(); }
    std::shared_ptr<Performance> operator[](int i) const { return scores[(size_t)i]; }
    void add(std::shared_ptr<Performance> p) { scores.push_back(p); }
    // ten lines, "Mean <name, left-aligned to 13>: <mean>% (+/- <population stdev>%)": prevalence, bias, recall, precision, F1,
    // specificity, accuracy, informedness, markededness (the reference's spelling), MCC -- to `out` only (the caller prints)
    void outputMeanPerformance(std::ostream& out) const;
};

}  // namespace ml
}  // namespace portcullis
