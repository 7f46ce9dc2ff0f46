// ModelBundle: what `filt --self_train` trains beside its forest and `filt --model_file` needs to score with that forest faithfully -- the
// L95 intron threshold and the eight Markov models -- as one file (<prefix>.selftrain.models, or <prefix>.models of `train --markov`).
// The reference has no such file: a saved forest is applied there with L95 = 0 and untrained models.  The format is this project's own,
// little-endian, 752 612 bytes:
//   "PJBMODL1" | u32 L95 | u32 order (5) | u32 pw_len (32) | i32 sizes[8] | f64 tables[6 x 3125 x 5 + 2 x 32 x 5]
// sizes and tables in the order of pjb_markov_models: exon, intron, donor_t, donor_f, acceptor_t, acceptor_f (k-mer models of order 5,
// [context][next base] over A C G T N), donor_pw, acceptor_pw (position models, [position][base]).  A row holds the probabilities of the
// five bases behind a context (at a position), or five zeros if it was never trained; a size counts the rows that are not zero.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../bam/bam_master.hpp"

namespace portcullis {
namespace ml {

struct ModelBundleException : public PortcullisException {
    explicit ModelBundleException(const std::string& m) : PortcullisException(m) {}
};

struct ModelBundle {
    static constexpr size_t KMER_MODELS = 6, POS_MODELS = 2, KMER_TABLE = 3125 * 5, POS_TABLE = 32 * 5;
    static constexpr size_t TABLE_DOUBLES = KMER_MODELS * KMER_TABLE + POS_MODELS * POS_TABLE;
    static constexpr size_t FILE_BYTES = 8 + 3 * 4 + 8 * 4 + TABLE_DOUBLES * 8;

    uint32_t L95 = 0;
    int32_t sizes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<double> tables = std::vector<double>(TABLE_DOUBLES, 0.0);  // untrained: all zero

    const double* table(size_t model) const { return tables.data() + (model < KMER_MODELS ? model * KMER_TABLE : KMER_MODELS * KMER_TABLE + (model - KMER_MODELS) * POS_TABLE); }
    double* table(size_t model) { return const_cast<double*>(static_cast<const ModelBundle*>(this)->table(model)); }
    void countSizes();  // sizes[] from the tables

    std::string bytes() const;
    void save(const std::string& path) const;  // throws ModelBundleException if the file cannot be written
    // Host arithmetic only: "" if `bytes` is a bundle that can be scored with, else the fault in words.  Checked: the magic, the length,
    // order 5 and pw_len 32, every value finite and within [0, 1], every row summing to 0 or to 1 within 1e-12, every size equal to
    // the number of rows that are not zero.
    static std::string check(const std::string& bytes);
    // reads and checks (before a device is opened); throws ModelBundleException naming the file and the fault
    static ModelBundle load(const std::string& path);
};

}  // namespace ml
}  // namespace portcullis
