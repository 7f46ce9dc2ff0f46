// The few file-system questions the modes ask before they start (train, filt, self-training's rule directory).
#pragma once

#include <sys/stat.h>

#include <string>

namespace portcullis {

inline bool exists(const std::string& p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}
inline bool isDirectory(const std::string& p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
inline bool createDirectories(const std::string& p) {
    std::string cur;
    for (size_t i = 0; i <= p.size(); i++) {
        if (i == p.size() || p[i] == '/') {
            if (!cur.empty() && !exists(cur) && mkdir(cur.c_str(), 0777) != 0 && !exists(cur)) return false;
        }
        if (i < p.size()) cur.push_back(p[i]);
    }
    return isDirectory(p);
}

}  // namespace portcullis
