// strawberry_amd/csrc/gtf_host.h -- what the two forms of the GTF reader share on the host (gtf_host.cpp, gtf_api.hip): the
// handle, and the step from a file's transcripts to the annotation -- chromosome ids, the transcripts' order, the loci, the
// CSR arrays, the names and the segments.  Free of HIP.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/sbgpu.h"

struct sbgpu_gtf {
   // the annotation (sbgpu_annotation_t), the clusters, per isoform its exonic length and strand
   std::vector<int64_t> iso_off, exon_off, seg_off;
   std::vector<uint32_t> exon_left, exon_right, seg_left, seg_right;
   std::vector<int32_t> c_ref;
   std::vector<uint32_t> c_left, c_right;
   std::vector<uint8_t> c_strand;
   std::vector<int32_t> iso_len;
   std::vector<uint8_t> iso_strand;
   // the names: offsets and bytes
   std::vector<int64_t> gene_id_off, gene_name_off, tx_id_off, chrom_off;
   std::string gene_id, gene_name, tx_id, chrom;
   std::vector<uint8_t> line_status;
   int64_t info[16] = {};
   sbgpu_annotation_t annot{};
   sbgpu_clusters_t clusters{};
   sbgpu_gtf_names_t names{};
};

namespace sb {

// A transcript as a form found it: its first line in the file, that line's names (bytes somewhere that outlives the call to
// gtf_finish), its strand, its exons sorted, merged and disjoint, and how many exons the merge took away.
struct GtfRawTx {
   int64_t first_line;
   const uint8_t *chrom, *gene, *tx, *gname;
   int32_t l_chrom, l_gene, l_tx, l_gname;
   uint8_t strand;
   const uint32_t *xl, *xr;
   int64_t n_exons, merges;
};

// The lines' statuses (moved in) and the transcripts, in any order -> the handle's arrays.  SBGPU_OK, or a failure that
// api_fail has recorded under `who`.
int gtf_finish(const std::string &who, std::vector<GtfRawTx> &raw, std::vector<uint8_t> &&line_status, const sbgpu_gtf_opts_t *opts, sbgpu_gtf *g);
// the options as every form checks them
int gtf_check_opts(const std::string &who, const sbgpu_gtf_opts_t *opts);

} // namespace sb
