// strawberry_amd/csrc/splice_host.cpp -- sbgpu_splice_events_shapes_host / sbgpu_splice_events_build_host / sbgpu_splice_psi_host /
// sbgpu_splice_support_host (include/sbgpu.h): the event table of an annotation, and the one CPU statement of what
// csrc/splice_device.h computes from it -- the sums and the quotient are splice_rules.h's, and the kernels call the same functions.
// The table is annotation-only work, done once per annotation: it stays on the host.  No kernels and no HIP here: a plain C++
// compiler takes this file beside a main that supplies sb::api_fail.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "splice_rules.h"

namespace sb {
int api_fail(int code, const std::string &msg);

namespace {

struct SplTable {
   std::vector<int64_t> event_off, incl_off, incl_exon;
   std::vector<int32_t> event_locus, n_span, incl_iso;
   std::vector<uint8_t> event_kind, event_flags;
   std::vector<uint32_t> event_left, event_right, iso_left, iso_right;
   int64_t n_loci = 0, n_iso = 0, n_exons = 0;
};

// one exon or intron of one isoform, before the distinct ones are made events
struct SplPiece {
   uint32_t left, right;
   uint8_t kind, where; // where: SBGPU_SPLICE_FIRST / LAST / INTERNAL bits of an exon inside its isoform
   int32_t iso;         // inside the locus
   int64_t exon;        // global index of the exon, or of the exon upstream of the intron
};

int spl_build(const std::string &who, const sbgpu_annotation_t *annot, SplTable *t)
{
   if (!annot) return api_fail(SBGPU_EINVAL, who + ": null argument");
   const int64_t nl = annot->n_loci;
   if (nl < 0 || !annot->iso_off || !annot->exon_off) return api_fail(SBGPU_EINVAL, who + ": null offsets, or a negative locus count");
   if (nl > INT32_MAX) return api_fail(SBGPU_EINVAL, who + ": more than 2^31 - 1 loci");
   if (annot->iso_off[0] != 0) return api_fail(SBGPU_EINVAL, who + ": iso_off does not start at 0");
   for (int64_t l = 0; l < nl; ++l) {
      if (annot->iso_off[l + 1] < annot->iso_off[l]) return api_fail(SBGPU_EINVAL, who + ": the annotation's isoform offsets descend");
      if (annot->iso_off[l + 1] - annot->iso_off[l] > INT32_MAX) return api_fail(SBGPU_EINVAL, who + ": a locus of more than 2^31 - 1 isoforms");
   }
   const int64_t n_iso = annot->iso_off[nl];
   if (annot->exon_off[0] != 0) return api_fail(SBGPU_EINVAL, who + ": exon_off does not start at 0");
   for (int64_t j = 0; j < n_iso; ++j)
      if (annot->exon_off[j + 1] < annot->exon_off[j]) return api_fail(SBGPU_EINVAL, who + ": the annotation's exon offsets descend");
   const int64_t n_exons = annot->exon_off[n_iso];
   if (n_exons && (!annot->exon_left || !annot->exon_right)) return api_fail(SBGPU_EINVAL, who + ": the annotation's exons are needed");
   const uint32_t *XL = annot->exon_left, *XR = annot->exon_right;
   for (int64_t j = 0; j < n_iso; ++j)
      for (int64_t e = annot->exon_off[j]; e < annot->exon_off[j + 1]; ++e)
         if (XR[e] < XL[e] || (e > annot->exon_off[j] && XL[e] <= XR[e - 1]))
            return api_fail(SBGPU_EINVAL, who + ": the exons of an isoform are not ascending and disjoint");
   t->n_loci = nl, t->n_iso = n_iso, t->n_exons = n_exons;
   t->event_off.assign((size_t)nl + 1, 0), t->incl_off.assign(1, 0);
   t->iso_left.assign((size_t)n_iso, 0xFFFFFFFFu), t->iso_right.assign((size_t)n_iso, 0u);
   std::vector<SplPiece> pieces;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t j0 = annot->iso_off[l], j1 = annot->iso_off[l + 1];
      pieces.clear();
      for (int64_t j = j0; j < j1; ++j) {
         const int64_t e0 = annot->exon_off[j], e1 = annot->exon_off[j + 1];
         if (e0 == e1) continue;
         t->iso_left[(size_t)j] = XL[e0], t->iso_right[(size_t)j] = XR[e1 - 1];
         for (int64_t e = e0; e < e1; ++e) {
            const uint8_t where = (uint8_t)((e == e0 ? SBGPU_SPLICE_FIRST : 0) | (e == e1 - 1 ? SBGPU_SPLICE_LAST : 0));
            pieces.push_back({XL[e], XR[e], kSplExon, (uint8_t)(where ? where : SBGPU_SPLICE_INTERNAL), (int32_t)(j - j0), e});
            if (e + 1 < e1 && XL[e + 1] - XR[e] >= 2) pieces.push_back({XR[e] + 1, XL[e + 1] - 1, kSplIntron, 0, (int32_t)(j - j0), e});
         }
      }
      // (left, right, kind), then ascending isoform: an isoform owns an exon or an intron once, so the order is total
      std::sort(pieces.begin(), pieces.end(), [](const SplPiece &p, const SplPiece &q) {
         if (p.left != q.left) return p.left < q.left;
         if (p.right != q.right) return p.right < q.right;
         if (p.kind != q.kind) return p.kind < q.kind;
         return p.iso < q.iso;
      });
      const size_t u0 = t->event_kind.size();
      for (size_t i = 0; i < pieces.size();) {
         size_t k = i;
         uint8_t flags = 0;
         for (; k < pieces.size() && pieces[k].left == pieces[i].left && pieces[k].right == pieces[i].right && pieces[k].kind == pieces[i].kind; ++k) {
            flags |= pieces[k].where;
            t->incl_iso.push_back(pieces[k].iso), t->incl_exon.push_back(pieces[k].exon);
         }
         t->event_locus.push_back((int32_t)l), t->event_kind.push_back(pieces[i].kind), t->event_flags.push_back(flags);
         t->event_left.push_back(pieces[i].left), t->event_right.push_back(pieces[i].right);
         t->incl_off.push_back((int64_t)t->incl_iso.size());
         int32_t span = 0;
         for (int64_t j = j0; j < j1; ++j) span += spl_spans(t->iso_left[(size_t)j], t->iso_right[(size_t)j], pieces[i].left, pieces[i].right);
         t->n_span.push_back(span);
         i = k;
      }
      // SKIPPED / RETAINED: an exon event inside a distinct intron of the locus, an intron event inside a distinct exon
      const size_t u1 = t->event_kind.size();
      for (size_t u = u0; u < u1; ++u)
         for (size_t w = u0; w < u1; ++w)
            if (t->event_kind[w] != t->event_kind[u] && t->event_left[w] <= t->event_left[u] && t->event_right[u] <= t->event_right[w]) {
               t->event_flags[u] |= t->event_kind[u] == kSplExon ? SBGPU_SPLICE_SKIPPED : SBGPU_SPLICE_RETAINED;
               break;
            }
      t->event_off[(size_t)l + 1] = (int64_t)u1;
   }
   return SBGPU_OK;
}

// The table as the host forms need it
int spl_check(const std::string &who, const sbgpu_splice_events_t *t)
{
   if (!t) return api_fail(SBGPU_EINVAL, who + ": null argument");
   const int64_t nl = t->n_loci, nu = t->n_events, ni = t->n_incl;
   if (nl < 0 || t->n_iso < 0 || t->n_exons < 0 || nu < 0 || ni < 0) return api_fail(SBGPU_EINVAL, who + ": a negative count in the table");
   if (!t->event_off || !t->incl_off || !t->iso_off) return api_fail(SBGPU_EINVAL, who + ": the table's offsets are needed");
   if (nu && (!t->event_locus || !t->event_kind || !t->event_left || !t->event_right)) return api_fail(SBGPU_EINVAL, who + ": the table's events are needed");
   if (ni && (!t->incl_iso || !t->incl_exon)) return api_fail(SBGPU_EINVAL, who + ": the table's inclusion lists are needed");
   if (t->n_iso && (!t->iso_left || !t->iso_right)) return api_fail(SBGPU_EINVAL, who + ": the table's isoform extents are needed");
   if (t->event_off[0] != 0 || t->event_off[nl] != nu) return api_fail(SBGPU_EINVAL, who + ": event_off does not run from 0 to n_events");
   if (t->iso_off[0] != 0 || t->iso_off[nl] != t->n_iso) return api_fail(SBGPU_EINVAL, who + ": iso_off does not run from 0 to n_iso");
   if (t->incl_off[0] != 0 || t->incl_off[nu] != ni) return api_fail(SBGPU_EINVAL, who + ": incl_off does not run from 0 to n_incl");
   for (int64_t l = 0; l < nl; ++l) {
      if (t->event_off[l + 1] < t->event_off[l]) return api_fail(SBGPU_EINVAL, who + ": the table's event offsets descend");
      if (t->iso_off[l + 1] < t->iso_off[l]) return api_fail(SBGPU_EINVAL, who + ": the table's isoform offsets descend");
   }
   for (int64_t u = 0; u < nu; ++u) {
      if (t->incl_off[u + 1] < t->incl_off[u]) return api_fail(SBGPU_EINVAL, who + ": the table's inclusion offsets descend");
      const int64_t l = t->event_locus[u];
      if (l < 0 || l >= nl) return api_fail(SBGPU_EINVAL, who + ": an event_locus outside the loci");
      const int64_t niso = t->iso_off[l + 1] - t->iso_off[l];
      for (int64_t i = t->incl_off[u]; i < t->incl_off[u + 1]; ++i) {
         if (t->incl_iso[i] < 0 || t->incl_iso[i] >= niso) return api_fail(SBGPU_EINVAL, who + ": an incl_iso outside its locus");
         if (t->incl_exon[i] < 0 || t->incl_exon[i] >= t->n_exons) return api_fail(SBGPU_EINVAL, who + ": an incl_exon outside the exons");
      }
   }
   return SBGPU_OK;
}

} // namespace
} // namespace sb

using sb::api_fail;

extern "C" int sbgpu_splice_events_shapes_host(const sbgpu_annotation_t *annot, int64_t out[2])
{
   const std::string who = "sbgpu_splice_events_shapes_host";
   if (!out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   sb::SplTable t;
   if (const int rc = sb::spl_build(who, annot, &t); rc != SBGPU_OK) return rc;
   out[0] = (int64_t)t.event_kind.size(), out[1] = (int64_t)t.incl_iso.size();
   return SBGPU_OK;
}

extern "C" int sbgpu_splice_events_build_host(const sbgpu_annotation_t *annot, sbgpu_splice_events_t *out)
{
   const std::string who = "sbgpu_splice_events_build_host";
   if (!out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   sb::SplTable t;
   if (const int rc = sb::spl_build(who, annot, &t); rc != SBGPU_OK) return rc;
   const int64_t nu = (int64_t)t.event_kind.size(), ni = (int64_t)t.incl_iso.size();
   if (out->n_events != nu || out->n_incl != ni)
      return api_fail(SBGPU_EINVAL, who + ": n_events / n_incl are not this annotation's (size the arrays by sbgpu_splice_events_shapes_host)");
   if (!out->event_off || !out->incl_off || !out->iso_off || (nu && (!out->event_locus || !out->event_kind || !out->event_left || !out->event_right ||
                                                                      !out->event_flags || !out->n_span)) ||
       (ni && (!out->incl_iso || !out->incl_exon)) || (t.n_iso && (!out->iso_left || !out->iso_right)))
      return api_fail(SBGPU_EINVAL, who + ": a null array in the table to fill");
   out->n_loci = t.n_loci, out->n_iso = t.n_iso, out->n_exons = t.n_exons;
   std::copy(t.event_off.begin(), t.event_off.end(), out->event_off);
   std::copy(t.incl_off.begin(), t.incl_off.end(), out->incl_off);
   std::copy(annot->iso_off, annot->iso_off + t.n_loci + 1, out->iso_off);
   if (nu) {
      std::copy(t.event_locus.begin(), t.event_locus.end(), out->event_locus);
      std::copy(t.event_kind.begin(), t.event_kind.end(), out->event_kind);
      std::copy(t.event_left.begin(), t.event_left.end(), out->event_left);
      std::copy(t.event_right.begin(), t.event_right.end(), out->event_right);
      std::copy(t.event_flags.begin(), t.event_flags.end(), out->event_flags);
      std::copy(t.n_span.begin(), t.n_span.end(), out->n_span);
   }
   if (ni) {
      std::copy(t.incl_iso.begin(), t.incl_iso.end(), out->incl_iso);
      std::copy(t.incl_exon.begin(), t.incl_exon.end(), out->incl_exon);
   }
   if (t.n_iso) {
      std::copy(t.iso_left.begin(), t.iso_left.end(), out->iso_left);
      std::copy(t.iso_right.begin(), t.iso_right.end(), out->iso_right);
   }
   return SBGPU_OK;
}

extern "C" int sbgpu_splice_psi_host(const sbgpu_splice_events_t *t, int64_t n_rows, const double *x, const int32_t *keep, double *psi,
                                     int32_t *defined_count)
{
   const std::string who = "sbgpu_splice_psi_host";
   if (const int rc = sb::spl_check(who, t); rc != SBGPU_OK) return rc;
   if (n_rows < 0) return api_fail(SBGPU_EINVAL, who + ": a negative row count");
   const int64_t nu = t->n_events, n_iso = t->n_iso;
   if (n_rows && n_iso && !x) return api_fail(SBGPU_EINVAL, who + ": x is needed");
   if (n_rows && nu && !psi) return api_fail(SBGPU_EINVAL, who + ": psi is needed");
   for (int64_t u = 0; u < nu; ++u) {
      const int64_t j0 = t->iso_off[t->event_locus[u]], niso = t->iso_off[t->event_locus[u] + 1] - j0;
      const int64_t i0 = t->incl_off[u], n_incl = t->incl_off[u + 1] - i0;
      int32_t defined = 0;
      for (int64_t k = 0; k < n_rows; ++k) {
         const sb::SplPsi r = sb::spl_psi_row(x + k * n_iso + j0, keep ? keep + k * n_iso + j0 : nullptr, t->iso_left + j0, t->iso_right + j0, niso,
                                              t->event_left[u], t->event_right[u], t->incl_iso + i0, n_incl);
         psi[k * nu + u] = r.psi;
         defined += r.defined;
      }
      if (defined_count) defined_count[u] = defined;
   }
   return SBGPU_OK;
}

extern "C" int sbgpu_splice_support_host(const sbgpu_splice_events_t *t, const double *exon_bases, const double *junction_mass, double *support)
{
   const std::string who = "sbgpu_splice_support_host";
   if (const int rc = sb::spl_check(who, t); rc != SBGPU_OK) return rc;
   if (t->n_events && !support) return api_fail(SBGPU_EINVAL, who + ": support is needed");
   for (int64_t u = 0; u < t->n_events; ++u) {
      const int64_t i0 = t->incl_off[u];
      support[u] = sb::spl_support(t->event_kind[u] == sb::kSplExon ? exon_bases : junction_mass, t->incl_exon + i0, t->incl_off[u + 1] - i0);
   }
   return SBGPU_OK;
}
