#include "fasta.h"

#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace std;

namespace fplh {

bool load_fasta_contigs(const string& path, map<string, string>& contigs, string& err) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
        err = "There is a problem with the provided fasta file: could NOT read " + path;
        return false;
    }
    string data;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.append(buf, n);
    fclose(f);
    /* FastaReader's constructor + readNext + readAll, src/fastareader.cpp:5-101, restated on the bytes of the file:
       the constructor skips to the first '>' (wherever it is); from then on a record ends where a LINE starts with
       '>' -- a '>' inside a header or a sequence line is an ordinary character.  Of every line the first character
       is taken by get() (upper-cased, otherwise as it is -- even a line feed, when the line is empty) and the rest by
       getline(), which goes to the header for the first line and through str_keep_valid_sequence (upper case,
       letters / '-' / '*' only) for the others. */
    size_t i = data.find('>');
    bool eof = i == string::npos;
    if (!eof) i++;
    while (!eof) {
        string header, seq;
        bool foundHeader = false;
        for (;;) {
            if (i >= data.size()) {
                eof = true;
                break;
            }
            char c = data[i++];
            if (c == '>') break;
            if (foundHeader) {
                if (c >= 'a' && c <= 'z') c -= ('a' - 'A');
                seq += c;
            } else {
                header += c;
            }
            const size_t e = data.find('\n', i);
            const string line = data.substr(i, (e == string::npos ? data.size() : e) - i);
            i = e == string::npos ? data.size() : e + 1;
            if (!foundHeader) {
                header += line;
                foundHeader = true;
            } else {
                for (char ch : line) {
                    if (ch >= 'a' && ch <= 'z') ch -= ('a' - 'A');
                    if (isalpha((unsigned char)ch) || ch == '-' || ch == '*') seq += ch;
                }
            }
        }
        contigs[header] = seq;
    }
    return true;
}

bool load_fasta_adapters(const string& path, vector<string>& adapters, ostream* log, string& err) {
    map<string, string> contigs;
    if (!load_fasta_contigs(path, contigs, err)) return false;
    for (auto& kv : contigs) { /* Options::loadFastaAdapters, src/options.cpp:50-59 */
        if (kv.second.length() >= 6) adapters.push_back(kv.second);
        else if (log) *log << "skip too short adapter sequence in " << path << " (6bp required): " << kv.second << endl;
    }
    return true;
}

}  // namespace fplh

/* test hook: "header\tsequence\n" for every contig in map order; malloc'ed, free with fplh_free */
extern "C" int fplh_load_fasta(const char* path, char** out, unsigned long long* out_len) {
    std::map<std::string, std::string> contigs;
    std::string err;
    if (!fplh::load_fasta_contigs(path, contigs, err)) return -1;
    std::string o;
    for (auto& kv : contigs) o += kv.first + "\t" + kv.second + "\n";
    *out = (char*)malloc(o.size() + 1);
    memcpy(*out, o.data(), o.size());
    *out_len = o.size();
    return (int)contigs.size();
}
