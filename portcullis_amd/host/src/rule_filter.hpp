// RuleFilter: the rule files of `filt --filter_file` -- a JSON object with "parameters" (key -> operator and value) and a boolean
// "expression" over the keys -- evaluated over the text of a junction table, with no pandas and no Python.  What a rule means is what
// the reference's rule_filter.py makes of it (scripts/portcullis/portcullis/rule_filter.py:45-110, json2pandas, and read_csv at :341):
//   * operators gt gte eq lt lte in "not in"; a key `name.N` (one digit) addresses column `name`, so a column can be tested twice;
//   * the expression holds keys, & | and parentheses; & binds tighter than |, as in Python;
//   * a column is numeric when every one of its values is a number (or one of pandas' missing-value spellings), else it holds strings;
//     a string column takes eq, in and not in; a missing value fails every test but "not in";
//   * every column of the table's header but the first (the index) can be addressed.
// The expression is parsed here, never substituted into program text.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include <portcullis/bam/bam_master.hpp>

namespace portcullis {

struct RuleFilterException : public PortcullisException {
    explicit RuleFilterException(const std::string& m) : PortcullisException(m) {}
};

class RuleFilter {
public:
    enum class Op { GT, GTE, EQ, LT, LTE, IN, NOT_IN };
    struct Value {  // a JSON string, or a number (true / false: 1 / 0)
        bool isString = false;
        std::string s;
        double d = 0.0;
    };
    struct Parameter {
        std::string key, column;
        Op op = Op::EQ;
        std::vector<Value> values;  // one, or the list of in / not in
        size_t columnIndex = 0;
    };
    struct Node {  // expression tree: a parameter, or & / | of two subtrees
        char kind = 'p';
        size_t parameter = 0;
        std::unique_ptr<Node> a, b;
    };

private:
    std::vector<Parameter> parameters;
    std::vector<std::string> expressionKeys;
    std::unique_ptr<Node> root;

public:
    // Reads and checks the file: throws RuleFilterException with the script's messages for a faulty configuration, an unknown
    // operator, an expression key without a parameter (and its own for text that is not JSON or an expression that cannot be parsed).
    static RuleFilter load(const std::string& path);
    static RuleFilter parse(const std::string& json);
    // fieldnames: the table's columns; rows: their text, one vector per junction.  Throws for a parameter on an unknown column.
    std::vector<char> evaluate(const std::vector<std::string>& fieldnames, const std::vector<std::vector<std::string>>& rows);
};

}  // namespace portcullis
