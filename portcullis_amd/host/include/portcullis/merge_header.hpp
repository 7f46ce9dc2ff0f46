// The header of a merged BAM (`portcullis_amd prep --merge`) from the headers of its inputs, as a pure function: strings in,
// a string out, no file and no device -- tests/cpp/merge_header.cc runs it on its own.
//   - every input must have the first input's reference dictionary (count, names, lengths: the BAM header's binary table);
//   - the text is the first input's, its @HD line saying SO:coordinate (the field is replaced or appended; a file without @HD
//     gets one);
//   - the @RG, @PG and @CO lines of later inputs follow in input order, unless a byte-identical line is there already;
//   - two different @RG (or @PG) lines with one ID are refused: read groups are not renamed.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace portcullis {

struct BamHeaderInfo {
    std::string file;                // (for messages)
    std::string text;                // the SAM header text
    std::vector<std::string> names;  // the reference dictionary
    std::vector<int32_t> lens;
};

class MergeHeaderException : public std::runtime_error {
public:
    explicit MergeHeaderException(const std::string& what) : std::runtime_error(what) {}
};

namespace merge_header_detail {
inline std::vector<std::string> lines(const std::string& text) {
    std::vector<std::string> out;
    size_t at = 0;
    while (at < text.size()) {
        size_t nl = text.find('\n', at);
        if (nl == std::string::npos) nl = text.size();
        if (nl > at) out.push_back(text.substr(at, nl - at));
        at = nl + 1;
    }
    return out;
}
// the value of a line's ID field ("" if it has none)
inline std::string idOf(const std::string& line) {
    size_t at = 0;
    while ((at = line.find('\t', at)) != std::string::npos) {
        at++;
        if (line.compare(at, 3, "ID:") == 0) {
            const size_t end = line.find('\t', at);
            return line.substr(at + 3, end == std::string::npos ? std::string::npos : end - at - 3);
        }
    }
    return "";
}
// an @HD line that says SO:coordinate
inline std::string sortedHd(const std::string& hd) {
    std::string out;
    bool seen = false;
    size_t at = 0;
    while (at <= hd.size()) {
        size_t tab = hd.find('\t', at);
        if (tab == std::string::npos) tab = hd.size();
        std::string field = hd.substr(at, tab - at);
        if (field.compare(0, 3, "SO:") == 0) {
            field = "SO:coordinate";
            seen = true;
        }
        if (at) out += '\t';
        out += field;
        at = tab + 1;
    }
    if (!seen) out += "\tSO:coordinate";
    return out;
}
}  // namespace merge_header_detail

// Refuses inputs whose dictionaries differ: the message names the file and the first target that differs.
inline void checkSameDictionary(const std::vector<BamHeaderInfo>& in) {
    for (size_t f = 1; f < in.size(); f++) {
        const BamHeaderInfo &a = in[0], &b = in[f];
        const size_t n = std::min(a.names.size(), b.names.size());
        for (size_t t = 0; t < n; t++) {
            if (a.names[t] != b.names[t])
                throw MergeHeaderException("The BAM files do not share one reference dictionary: target " + std::to_string(t) + " is " + b.names[t] + " in " + b.file +
                                           " and " + a.names[t] + " in " + a.file);
            if (a.lens[t] != b.lens[t])
                throw MergeHeaderException("The BAM files do not share one reference dictionary: target " + std::to_string(t) + " (" + a.names[t] + ") has " +
                                           std::to_string(b.lens[t]) + " bases in " + b.file + " and " + std::to_string(a.lens[t]) + " in " + a.file);
        }
        if (a.names.size() != b.names.size()) {
            const BamHeaderInfo& more = a.names.size() > n ? a : b;
            throw MergeHeaderException("The BAM files do not share one reference dictionary: " + b.file + " has " + std::to_string(b.names.size()) + " targets and " +
                                       a.file + " has " + std::to_string(a.names.size()) + " (target " + std::to_string(n) + ", " + more.names[n] + ", is missing in one)");
        }
    }
}

inline std::string mergeBamHeaders(const std::vector<BamHeaderInfo>& in) {
    using namespace merge_header_detail;
    if (in.empty()) return "";
    checkSameDictionary(in);
    std::vector<std::string> out = lines(in[0].text);
    if (!out.empty() && out[0].compare(0, 3, "@HD") == 0) out[0] = sortedHd(out[0]);
    else out.insert(out.begin(), "@HD\tVN:1.4\tSO:coordinate");
    for (size_t f = 1; f < in.size(); f++)
        for (const std::string& line : lines(in[f].text)) {
            const std::string kind = line.substr(0, 3);
            if (kind != "@RG" && kind != "@PG" && kind != "@CO") continue;
            bool there = false;
            for (const std::string& have : out)
                if (have == line) there = true;
            if (there) continue;
            if (kind != "@CO") {
                const std::string id = idOf(line);
                for (const std::string& have : out)
                    if (have.compare(0, 3, kind) == 0 && idOf(have) == id)
                        throw MergeHeaderException("The BAM files have two different " + kind + " lines with ID " + id + " (the second in " + in[f].file +
                                                   "): read groups and programs are not renamed.  Give them distinct IDs first (samtools addreplacerg / reheader).");
            }
            out.push_back(line);
        }
    std::string text;
    for (const std::string& line : out) text += line + "\n";
    return text;
}

}  // namespace portcullis
