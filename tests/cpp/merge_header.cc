// The header of a merged BAM (portcullis/merge_header.hpp: mergeBamHeaders, checkSameDictionary) on strings written out by hand.
// Stand-alone host program: tests/test_host_merge_header.py builds it with the address and undefined-behaviour sanitizers linked
// in and runs it.
#include <portcullis/merge_header.hpp>

#include <cstdio>

using namespace portcullis;
using std::string;

static int g_checks = 0, g_failed = 0;
static void checkEq(const string& got, const string& want, const char* what, int line) {
    g_checks++;
    if (got != want) {
        g_failed++;
        fprintf(stderr, "%s:%d: %s is\n[%s]\nexpected\n[%s]\n", __FILE__, line, what, got.c_str(), want.c_str());
    }
}
#define CHECK_EQ(got, want) checkEq((got), (want), #got, __LINE__)
// the message of the refusal ("" if the call went through)
static string refusal(const std::vector<BamHeaderInfo>& in) {
    try {
        (void)mergeBamHeaders(in);
    } catch (const MergeHeaderException& e) {
        return e.what();
    }
    return "";
}
static void checkHas(const string& msg, const string& word, int line) {
    g_checks++;
    if (msg.find(word) == string::npos) {
        g_failed++;
        fprintf(stderr, "%s:%d: [%s] does not say [%s]\n", __FILE__, line, msg.c_str(), word.c_str());
    }
}
#define CHECK_HAS(msg, word) checkHas((msg), (word), __LINE__)

static const string SQ = "@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:500\n";
static BamHeaderInfo info(const string& file, const string& text) { return BamHeaderInfo{file, text, {"chr1", "chr2"}, {1000, 500}}; }

int main() {
    const string hd = "@HD\tVN:1.4\tSO:coordinate\n";
    // identical headers: the first file's text
    {
        const string t = hd + SQ + "@RG\tID:a\tSM:s\n@PG\tID:bwa\tPN:bwa\n@CO\thello\n";
        CHECK_EQ(mergeBamHeaders({info("a.bam", t), info("b.bam", t), info("c.bam", t)}), t);
        CHECK_EQ(mergeBamHeaders({info("a.bam", t)}), t);
    }
    // later @RG / @PG / @CO lines are appended once, in file order; @SQ and @HD of later files are not
    {
        const string a = hd + SQ + "@RG\tID:a\tSM:s\n@PG\tID:bwa\tPN:bwa\n";
        const string b = "@HD\tVN:1.6\tSO:unsorted\n" + SQ + "@RG\tID:b\tSM:s\n@RG\tID:a\tSM:s\n@PG\tID:bwa\tPN:bwa\n@CO\tfrom b\n";
        const string c = hd + SQ + "@CO\tfrom b\n@CO\tfrom c\n@RG\tID:b\tSM:s\n@PG\tID:star\tPN:STAR\n@RG\tID:c\tSM:t\n";
        CHECK_EQ(mergeBamHeaders({info("a.bam", a), info("b.bam", b), info("c.bam", c)}),
                 a + "@RG\tID:b\tSM:s\n@CO\tfrom b\n@CO\tfrom c\n@PG\tID:star\tPN:STAR\n@RG\tID:c\tSM:t\n");
    }
    // @HD: missing, tagged unsorted, without SO, SO in the middle; a text without a final newline; an empty text
    CHECK_EQ(mergeBamHeaders({info("a.bam", SQ)}), hd + SQ);
    CHECK_EQ(mergeBamHeaders({info("a.bam", "")}), hd);
    CHECK_EQ(mergeBamHeaders({info("a.bam", "@HD\tVN:1.5\tSO:unsorted\n" + SQ)}), "@HD\tVN:1.5\tSO:coordinate\n" + SQ);
    CHECK_EQ(mergeBamHeaders({info("a.bam", "@HD\tVN:1.5\n" + SQ)}), "@HD\tVN:1.5\tSO:coordinate\n" + SQ);
    CHECK_EQ(mergeBamHeaders({info("a.bam", "@HD\tVN:1.5\tSO:queryname\tGO:none\n" + SQ)}), "@HD\tVN:1.5\tSO:coordinate\tGO:none\n" + SQ);
    CHECK_EQ(mergeBamHeaders({info("a.bam", "@HD\tVN:1.5\tSO:unknown")}), "@HD\tVN:1.5\tSO:coordinate\n");
    // an ID with two meanings is refused, and named; the same ID on @RG and @PG is no collision
    {
        const string a = hd + SQ + "@RG\tID:x\tSM:one\n";
        string msg = refusal({info("a.bam", a), info("b.bam", hd + SQ + "@RG\tID:x\tSM:two\n")});
        CHECK_HAS(msg, "@RG");
        CHECK_HAS(msg, "ID x");
        CHECK_HAS(msg, "b.bam");
        msg = refusal({info("a.bam", hd + SQ + "@PG\tID:p\tPN:one\n"), info("b.bam", hd + SQ), info("c.bam", hd + SQ + "@PG\tID:p\tPN:two\tVN:2\n")});
        CHECK_HAS(msg, "@PG");
        CHECK_HAS(msg, "ID p");
        CHECK_HAS(msg, "c.bam");
        CHECK_EQ(refusal({info("a.bam", a), info("b.bam", hd + SQ + "@PG\tID:x\tPN:prog\n")}), "");
        CHECK_EQ(refusal({info("a.bam", a), info("b.bam", hd + SQ + "@RG\tID:xy\tSM:two\n")}), "");
    }
    // dictionaries: count, a name, a length -- the first differing target is named
    {
        const BamHeaderInfo a = info("a.bam", hd + SQ);
        BamHeaderInfo b = info("b.bam", hd + SQ);
        b.names.push_back("chr3");
        b.lens.push_back(70);
        string msg = refusal({a, a, b});
        CHECK_HAS(msg, "b.bam");
        CHECK_HAS(msg, "3 targets");
        CHECK_HAS(msg, "target 2");
        CHECK_HAS(msg, "chr3");
        msg = refusal({b, a});
        CHECK_HAS(msg, "a.bam has 2 targets");
        CHECK_HAS(msg, "chr3");
        BamHeaderInfo c = info("c.bam", hd + SQ);
        c.names[1] = "chrII";
        msg = refusal({a, c});
        CHECK_HAS(msg, "target 1 is chrII in c.bam");
        BamHeaderInfo d = info("d.bam", hd + SQ);
        d.lens[0] = 1001;
        d.names[1] = "other";
        msg = refusal({a, d});
        CHECK_HAS(msg, "target 0 (chr1) has 1001 bases in d.bam");
        // (the text's @SQ lines do not matter: the binary table does)
        CHECK_EQ(refusal({a, info("e.bam", hd + "@SQ\tSN:zzz\tLN:1\n")}), "");
    }
    printf("merge_header: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
