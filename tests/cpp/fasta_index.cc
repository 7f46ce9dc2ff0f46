// GenomeMapper's FASTA index writer and fetchBases, for tests/test_oracle_htslib_witness.py to hold against htslib.
//   fasta_index build FA   writes FA.fai (buildFastaIndex); exit status 1 and the message on stderr where the writer refuses
//   fasta_index fetch FA   reads "name beg end" lines on stdin, prints "len string" per line (fetchBases through FA.fai)
#include <portcullis/bam/genome_mapper.hpp>

#include <cstdio>
#include <cstring>
#include <string>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    portcullis::bam::GenomeMapper g(argv[2]);
    try {
        if (!strcmp(argv[1], "build")) {
            g.buildFastaIndex();
            return 0;
        }
        g.loadFastaIndex();
        char name[1024];
        int beg, end;
        while (scanf("%1023s %d %d", name, &beg, &end) == 3) {
            const std::string s = g.fetchBases(name, beg, end);
            printf("%zu %s\n", s.size(), s.c_str());
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
