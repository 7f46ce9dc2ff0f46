// The witness program of tests/golden/markov_witness.cc over the project's own portcullis/ml/markov_model.hpp (the include
// path of the build line decides which header <portcullis/ml/markov_model.hpp> is): same input, same output, so that
// tests/test_host_markov_witness.py can hold what it prints against what the reference's models printed.  Host code only,
// nothing of the GPU library; built with the address and undefined-behaviour sanitizers and run directly.
#include "../golden/markov_witness.cc"
