// Performance: see portcullis/ml/performance.hpp.
#include <portcullis/ml/performance.hpp>

#include <cmath>
#include <cstdio>
#include <iomanip>
#include <sstream>

namespace portcullis {
namespace ml {

double Performance::getFBScore(double beta) const {
    if (beta <= 0) return 0.0;
    const double recall = getRecall(), precision = getPrecision(), beta2 = beta * beta;
    const double below = (beta2 * precision) + recall;
    if (!(below > 0.0)) return 0.0;  // (the reference divides 0 by 0 here)
    return (1.0 + beta2) * (precision * recall) / below;
}

double Performance::getMCC() const {
    const double x = getInformedness() * getMarkedness();
    return x > 0.0 ? std::sqrt(x) : 0.0;  // (below 0 the reference's root is a NaN, at -0.0 it is -0.0)
}

std::string Performance::to_2dp_string(double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.2f", v);
    return buf;
}

std::string Performance::toLongString() const {
    std::string s = std::to_string(tp) + "\t" + std::to_string(tn) + "\t" + std::to_string(fp) + "\t" + std::to_string(fn);
    for (const double v : {getPrevalence(), getBias(), getSensitivity(), getSpecificity(), getPrecision(), getNPV(), getF1Score(), getAccuracy(),
                           getInformedness(), getMarkedness(), getMCC()})
        s += "\t" + to_2dp_string(v);
    return s;
}

void PerformanceList::outputMeanScore(const std::vector<double>& values, const std::string& name, std::ostream& out) {
    double sum = 0.0, sq_sum = 0.0;
    for (const double v : values) sum += v;
    for (const double v : values) sq_sum += v * v;
    const double n = (double)values.size(), mean = sum / n, var = sq_sum / n - mean * mean;
    const double stdev = var > 0.0 ? std::sqrt(var) : 0.0;  // (folds of one value: rounding can leave the difference just below 0)
    std::ostringstream msg;
    msg << "Mean " << std::left << std::setw(13) << name << ": " << std::fixed << std::setprecision(2) << mean << "% (+/- " << stdev << "%)\n";
    out << msg.str();
}

void PerformanceList::outputMeanPerformance(std::ostream& out) const {
    struct Column {
        const char* name;
        double (Performance::*get)() const;
    };
    static const Column columns[] = {{"prevalence", &Performance::getPrevalence},     {"bias", &Performance::getBias},
                                     {"recall", &Performance::getRecall},             {"precision", &Performance::getPrecision},
                                     {"F1", &Performance::getF1Score},                {"specificity", &Performance::getSpecificity},
                                     {"accuracy", &Performance::getAccuracy},         {"informedness", &Performance::getInformedness},
                                     {"markededness", &Performance::getMarkedness},   {"MCC", &Performance::getMCC}};
    for (const Column& c : columns) {
        std::vector<double> values;
        for (const auto& p : scores) values.push_back(((*p).*(c.get))());
        outputMeanScore(values, c.name, out);
    }
}

}  // namespace ml
}  // namespace portcullis
