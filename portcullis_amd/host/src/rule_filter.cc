// RuleFilter: see rule_filter.hpp.
#include "rule_filter.hpp"

#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <set>
#include <utility>

namespace portcullis {

namespace {

// ---- a small JSON reader: objects, arrays, strings, numbers, true / false / null
struct JVal {
    enum Type { Null, Bool, Num, Str, Arr, Obj } type = Null;
    bool b = false;
    double num = 0.0;
    std::string str;
    std::vector<JVal> arr;
    std::vector<std::pair<std::string, JVal>> obj;
    const JVal* get(const std::string& k) const {
        const JVal* hit = nullptr;
        for (const auto& kv : obj)
            if (kv.first == k) hit = &kv.second;  // (the last one wins, as in Python)
        return hit;
    }
};

struct JReader {
    const std::string& t;
    size_t at = 0;
    int depth = 0;
    [[noreturn]] void bad(const std::string& what) const {
        throw RuleFilterException("Could not read the filter configuration as JSON: " + what + " at offset " + std::to_string(at));
    }
    void ws() {
        while (at < t.size() && (t[at] == ' ' || t[at] == '\t' || t[at] == '\n' || t[at] == '\r')) at++;
    }
    static void utf8(std::string& o, unsigned cp) {
        if (cp < 0x80) o.push_back((char)cp);
        else if (cp < 0x800) {
            o.push_back((char)(0xC0 | (cp >> 6)));
            o.push_back((char)(0x80 | (cp & 0x3F)));
        } else if (cp < 0x10000) {
            o.push_back((char)(0xE0 | (cp >> 12)));
            o.push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
            o.push_back((char)(0x80 | (cp & 0x3F)));
        } else {
            o.push_back((char)(0xF0 | (cp >> 18)));
            o.push_back((char)(0x80 | ((cp >> 12) & 0x3F)));
            o.push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
            o.push_back((char)(0x80 | (cp & 0x3F)));
        }
    }
    unsigned hex4() {
        if (t.size() - at < 4) bad("a \\u escape that ends early");
        unsigned v = 0;
        for (int k = 0; k < 4; k++) {
            const char c = t[at++];
            v = v * 16 + (c >= '0' && c <= '9' ? (unsigned)(c - '0') : c >= 'a' && c <= 'f' ? (unsigned)(c - 'a' + 10) : c >= 'A' && c <= 'F' ? (unsigned)(c - 'A' + 10) : 256u);
            if (v > 0xFFFFu * 16u) bad("a \\u escape that is not hexadecimal");
        }
        if (v > 0xFFFF) bad("a \\u escape that is not hexadecimal");
        return v;
    }
    std::string string() {
        std::string o;
        at++;  // the opening quote
        while (true) {
            if (at >= t.size()) bad("a string without its closing quote");
            const char c = t[at++];
            if (c == '"') return o;
            if (c != '\\') {
                o.push_back(c);
                continue;
            }
            if (at >= t.size()) bad("a string without its closing quote");
            const char e = t[at++];
            switch (e) {
            case '"': o.push_back('"'); break;
            case '\\': o.push_back('\\'); break;
            case '/': o.push_back('/'); break;
            case 'b': o.push_back('\b'); break;
            case 'f': o.push_back('\f'); break;
            case 'n': o.push_back('\n'); break;
            case 'r': o.push_back('\r'); break;
            case 't': o.push_back('\t'); break;
            case 'u': {
                unsigned cp = hex4();
                if (cp >= 0xD800 && cp < 0xDC00 && t.compare(at, 2, "\\u") == 0) {
                    at += 2;
                    const unsigned lo = hex4();
                    cp = 0x10000 + ((cp - 0xD800) << 10) + ((lo - 0xDC00) & 0x3FF);
                }
                utf8(o, cp);
                break;
            }
            default: bad("an unknown escape in a string");
            }
        }
    }
    JVal value() {
        if (++depth > 64) bad("nesting deeper than 64 levels");
        ws();
        if (at >= t.size()) bad("the text ends where a value should be");
        JVal v;
        const char c = t[at];
        if (c == '{') {
            v.type = JVal::Obj;
            at++;
            ws();
            if (at < t.size() && t[at] == '}') at++;
            else
                while (true) {
                    ws();
                    if (at >= t.size() || t[at] != '"') bad("a key that is not a string");
                    std::string k = string();
                    ws();
                    if (at >= t.size() || t[at] != ':') bad("a key without ':'");
                    at++;
                    v.obj.emplace_back(std::move(k), value());
                    ws();
                    if (at < t.size() && t[at] == ',') {
                        at++;
                        continue;
                    }
                    if (at < t.size() && t[at] == '}') {
                        at++;
                        break;
                    }
                    bad("an object without ',' or '}'");
                }
        } else if (c == '[') {
            v.type = JVal::Arr;
            at++;
            ws();
            if (at < t.size() && t[at] == ']') at++;
            else
                while (true) {
                    v.arr.push_back(value());
                    ws();
                    if (at < t.size() && t[at] == ',') {
                        at++;
                        continue;
                    }
                    if (at < t.size() && t[at] == ']') {
                        at++;
                        break;
                    }
                    bad("an array without ',' or ']'");
                }
        } else if (c == '"') {
            v.type = JVal::Str;
            v.str = string();
        } else if (t.compare(at, 4, "true") == 0) {
            v.type = JVal::Bool, v.b = true, at += 4;
        } else if (t.compare(at, 5, "false") == 0) {
            v.type = JVal::Bool, v.b = false, at += 5;
        } else if (t.compare(at, 4, "null") == 0) {
            at += 4;
        } else if (c == '-' || (c >= '0' && c <= '9')) {
            size_t e = at + 1;
            while (e < t.size() && ((t[e] >= '0' && t[e] <= '9') || t[e] == '.' || t[e] == 'e' || t[e] == 'E' || t[e] == '+' || t[e] == '-')) e++;
            const std::string n = t.substr(at, e - at);
            char* end = nullptr;
            v.type = JVal::Num;
            v.num = strtod(n.c_str(), &end);
            if (end != n.c_str() + n.size()) bad("a number that cannot be read");
            at = e;
        } else
            bad("a value that is none of object, array, string, number, true, false, null");
        depth--;
        return v;
    }
};

const char* const FAULTY = "Configuration is faulty - please ensure that the JSON has valid \"parameters\" and \"expression\" fields.";

bool toValue(const JVal& j, RuleFilter::Value& v) {
    if (j.type == JVal::Str) {
        v.isString = true;
        v.s = j.str;
        return true;
    }
    if (j.type == JVal::Num || j.type == JVal::Bool) {
        v.d = j.type == JVal::Num ? j.num : (j.b ? 1.0 : 0.0);
        return true;
    }
    return false;
}

// the spellings of a missing value: the script's own list and the ones pandas adds to it
bool isMissing(const std::string& s) {
    static const std::set<std::string> na = {"", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "N/A", "NULL", "NaN",
                                             "n/a", "nan", "null", "<NA>", "NA", "None"};
    return na.count(s) != 0;
}

bool toNumber(const std::string& s, double& d) {
    if (s.empty()) return false;
    const char c = s[0];
    if (!((c >= '0' && c <= '9') || c == '-' || c == '+' || c == '.' || c == 'i' || c == 'I')) return false;
    if (s.find_first_of("xXpP") != std::string::npos) return false;  // (strtod would take hexadecimal floats)
    char* end = nullptr;
    errno = 0;
    d = strtod(s.c_str(), &end);
    return end == s.c_str() + s.size();
}

struct ExprParser {
    const std::vector<std::string>& tok;
    const std::vector<RuleFilter::Parameter>& params;
    size_t at = 0;
    [[noreturn]] void bad(const std::string& what) const { throw RuleFilterException("Could not read the filter's expression: " + what); }
    std::unique_ptr<RuleFilter::Node> join(char kind, std::unique_ptr<RuleFilter::Node> a, std::unique_ptr<RuleFilter::Node> b) {
        auto n = std::make_unique<RuleFilter::Node>();
        n->kind = kind;
        n->a = std::move(a);
        n->b = std::move(b);
        return n;
    }
    std::unique_ptr<RuleFilter::Node> atom() {
        if (at >= tok.size()) bad("it ends where a key or '(' should be");
        const std::string& t = tok[at];
        if (t == "(") {
            at++;
            auto n = orExpr();
            if (at >= tok.size() || tok[at] != ")") bad("a '(' without its ')'");
            at++;
            return n;
        }
        if (t == ")" || t == "&" || t == "|") bad("'" + t + "' where a key or '(' should be");
        auto n = std::make_unique<RuleFilter::Node>();
        for (size_t k = 0; k < params.size(); k++)
            if (params[k].key == t) n->parameter = k;
        at++;
        return n;
    }
    std::unique_ptr<RuleFilter::Node> andExpr() {
        auto n = atom();
        while (at < tok.size() && tok[at] == "&") {
            at++;
            n = join('&', std::move(n), atom());
        }
        return n;
    }
    std::unique_ptr<RuleFilter::Node> orExpr() {
        auto n = andExpr();
        while (at < tok.size() && tok[at] == "|") {
            at++;
            n = join('|', std::move(n), andExpr());
        }
        return n;
    }
};

}  // namespace

RuleFilter RuleFilter::load(const std::string& path) {
    std::ifstream in(path, std::ios::binary);
    if (!in.good()) throw RuleFilterException("Could not find filter configuration file at: " + path);
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    return parse(text);
}

RuleFilter RuleFilter::parse(const std::string& text) {
    JReader rd{text};
    const JVal top = rd.value();
    rd.ws();
    if (rd.at != text.size()) rd.bad("text after the value");
    const JVal* jp = top.type == JVal::Obj ? top.get("parameters") : nullptr;
    const JVal* je = top.type == JVal::Obj ? top.get("expression") : nullptr;
    if (!jp || !je || jp->type != JVal::Obj || je->type != JVal::Str) throw RuleFilterException(FAULTY);
    RuleFilter f;
    for (const auto& kv : jp->obj) {
        Parameter p;
        p.key = kv.first;
        p.column = p.key.substr(0, p.key.find('.'));
        const JVal* op = kv.second.type == JVal::Obj ? kv.second.get("operator") : nullptr;
        const JVal* val = kv.second.type == JVal::Obj ? kv.second.get("value") : nullptr;
        if (!op || !val) throw RuleFilterException(FAULTY);
        static const std::pair<const char*, Op> ops[] = {{"gt", Op::GT}, {"gte", Op::GTE}, {"eq", Op::EQ}, {"lt", Op::LT}, {"lte", Op::LTE}, {"in", Op::IN}, {"not in", Op::NOT_IN}};
        bool known = false;
        for (const auto& o : ops)
            if (op->type == JVal::Str && op->str == o.first) p.op = o.second, known = true;
        if (!known) throw RuleFilterException("Unrecognized operator for " + p.key + ": " + (op->type == JVal::Str ? op->str : std::string("(not a string)")));
        if (p.op == Op::IN || p.op == Op::NOT_IN) {
            if (val->type != JVal::Arr) throw RuleFilterException(FAULTY);
            for (const auto& e : val->arr) {
                Value v;
                if (!toValue(e, v)) throw RuleFilterException(FAULTY);
                p.values.push_back(v);
            }
        } else {
            Value v;
            if (!toValue(*val, v)) throw RuleFilterException(FAULTY);
            p.values.push_back(v);
        }
        bool replaced = false;  // (a key given twice: the last one wins)
        for (auto& q : f.parameters)
            if (q.key == p.key) q = p, replaced = true;
        if (!replaced) f.parameters.push_back(p);
    }
    // the expression's tokens: runs of anything but blanks and parentheses, and the parentheses
    std::vector<std::string> tok;
    const std::string& e = je->str;
    for (size_t i = 0; i < e.size();) {
        if (e[i] == ' ') i++;
        else if (e[i] == '(' || e[i] == ')') tok.push_back(std::string(1, e[i++]));
        else {
            size_t k = i;
            while (k < e.size() && e[k] != ' ' && e[k] != '(' && e[k] != ')') k++;
            tok.push_back(e.substr(i, k - i));
            i = k;
        }
    }
    std::string missing;
    for (const auto& t : tok) {
        if (t == "(" || t == ")" || t == "&" || t == "|") continue;
        f.expressionKeys.push_back(t);
        bool found = false;
        for (const auto& p : f.parameters) found = found || p.key == t;
        if (!found && missing.find("\n\t" + t + "\n") == std::string::npos && (missing.size() < t.size() + 2 || missing.compare(missing.size() - t.size() - 2, std::string::npos, "\n\t" + t) != 0))
            missing += "\n\t" + t;
    }
    if (!missing.empty()) throw RuleFilterException("Expression and required parameters mismatch:" + missing);
    ExprParser ep{tok, f.parameters};
    f.root = ep.orExpr();
    if (ep.at != tok.size()) ep.bad("'" + tok[ep.at] + "' where '&', '|' or the end should be");
    return f;
}

std::vector<char> RuleFilter::evaluate(const std::vector<std::string>& fieldnames, const std::vector<std::vector<std::string>>& rows) {
    std::string unknown, names;
    for (auto& p : parameters) {
        bool found = false;
        for (size_t k = 0; k < fieldnames.size(); k++)
            if (fieldnames[k] == p.column) p.columnIndex = k, found = true;
        if (!found) unknown += (unknown.empty() ? "" : ",") + p.column;
        names += "\n\t" + p.column;
    }
    if (!unknown.empty()) {
        std::string fields;
        for (const auto& n : fieldnames) fields += "\n\t" + n;
        throw RuleFilterException("Unrecognized parameters: " + unknown + "\nFieldnames:" + fields + "\nParameter names:" + names);
    }
    const size_t n = rows.size();
    // every parameter's truth per row
    std::vector<std::vector<char>> truth(parameters.size(), std::vector<char>(n, 0));
    for (size_t k = 0; k < parameters.size(); k++) {
        const Parameter& p = parameters[k];
        const size_t col = p.columnIndex;
        bool numeric = true;  // as read_csv decides: a column of numbers (and missing values), or of strings
        std::vector<double> num(n, 0.0);
        std::vector<char> missing(n, 0);
        for (size_t r = 0; r < n; r++) {
            const std::string& s = rows[r].at(col);
            if (isMissing(s)) missing[r] = 1;
            else if (!toNumber(s, num[r])) {
                numeric = false;
                break;
            }
        }
        if (!numeric) {
            if (p.op != Op::EQ && p.op != Op::IN && p.op != Op::NOT_IN)
                throw RuleFilterException("Parameter " + p.key + ": column " + p.column + " holds strings, which take the operators eq, in and not in");
            for (size_t r = 0; r < n; r++) missing[r] = isMissing(rows[r][col]) ? 1 : 0;
        } else
            for (const auto& v : p.values)
                if (v.isString && p.op != Op::EQ && p.op != Op::IN && p.op != Op::NOT_IN)
                    throw RuleFilterException("Parameter " + p.key + ": column " + p.column + " holds numbers and cannot be ordered against the string \"" + v.s + "\"");
        for (size_t r = 0; r < n; r++) {
            bool any = false;  // equal to one of the values
            if (!missing[r])
                for (const auto& v : p.values) any = any || (numeric ? (!v.isString && num[r] == v.d) : (v.isString && rows[r][col] == v.s));
            const double x = num[r], y = p.values.empty() ? 0.0 : p.values[0].d;
            bool t = false;
            switch (p.op) {
            case Op::EQ: t = any; break;
            case Op::IN: t = any; break;
            case Op::NOT_IN: t = !any; break;
            case Op::GT: t = !missing[r] && x > y; break;
            case Op::GTE: t = !missing[r] && x >= y; break;
            case Op::LT: t = !missing[r] && x < y; break;
            case Op::LTE: t = !missing[r] && x <= y; break;
            }
            truth[k][r] = t ? 1 : 0;
        }
    }
    std::vector<char> out(n, 0);
    struct Eval {
        const std::vector<std::vector<char>>& truth;
        bool run(const Node& nd, size_t r) const {
            if (nd.kind == 'p') return truth[nd.parameter][r] != 0;
            const bool a = run(*nd.a, r), b = run(*nd.b, r);
            return nd.kind == '&' ? (a && b) : (a || b);
        }
    } ev{truth};
    for (size_t r = 0; r < n; r++) out[r] = ev.run(*root, r) ? 1 : 0;
    return out;
}

}  // namespace portcullis
