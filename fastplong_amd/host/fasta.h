/*
 * fasta.h -- the FASTA reader behind --adapter_fasta.
 */
#ifndef FPLH_FASTA_H
#define FPLH_FASTA_H

#include <map>
#include <ostream>
#include <string>
#include <vector>

namespace fplh {

/* --adapter_fasta: FastaReader + Options::loadFastaAdapters (src/fastareader.cpp:5-101, src/options.cpp:39-66).
 * load_fasta_contigs restates the reader byte for byte (pinned against the real FastaReader, tests/test_host_split.py);
 * load_fasta_adapters keeps the sequences of >= 6 characters in header order -- the order trimByMultiSequences visits
 * them in -- and reports the skipped ones on `log` like the reference.  false + err when the file cannot be read. */
bool load_fasta_contigs(const std::string& path, std::map<std::string, std::string>& contigs, std::string& err);
bool load_fasta_adapters(const std::string& path, std::vector<std::string>& adapters, std::ostream* log, std::string& err);

}  // namespace fplh
#endif
