"""What sbgpu_plan_create makes of a batch's size classes before anything goes to the device (csrc/plan.cpp: pack_wide_rounds,
plan_arena_layout, stage_plan_head), from a stand-alone C++ program that is compiled together with plan.cpp -- it is free of
HIP -- with AddressSanitizer and UBSan: the wide loci's rounds against a restated first-fit-decreasing, the arena's offsets with
and without later phases, the staged class tables and lists against the classes.  No GPU, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""#include "plan.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static size_t up(size_t bytes) { return (bytes + 255) / 256 * 256; }
// entries (offset, bytes) in the order they were taken: aligned, ascending, behind each other, inside the arena
static bool laid_out(const std::vector<size_t> &off, const std::vector<size_t> &bytes, size_t total)
{
   for (size_t i = 0; i < off.size(); ++i) {
      if (off[i] % 256 || bytes[i] == 0) return false;
      if (off[i] + bytes[i] > (i + 1 < off.size() ? off[i + 1] : total)) return false;
   }
   return total % 256 == 0;
}

struct Batch {
   std::vector<int64_t> row_off{0}, iso_off{0}, f_off{0};
   void add(int64_t nrow, int64_t niso)
   {
      row_off.push_back(row_off.back() + nrow), iso_off.push_back(iso_off.back() + niso), f_off.push_back(f_off.back() + nrow * niso);
   }
   int64_t n() const { return (int64_t)row_off.size() - 1; }
   int64_t nrow(int32_t l) const { return row_off[(size_t)l + 1] - row_off[(size_t)l]; }
   int64_t niso(int32_t l) const { return iso_off[(size_t)l + 1] - iso_off[(size_t)l]; }
};

static int packing()
{
   const int n_cu = 8;
   // 65 isoforms: the layout of 80 columns holds 672 rows per workgroup -> 1, 2, 3, 5, 8 and 9 workgroups; tile loci in between
   Batch b;
   const int64_t rows65[6] = {100, 700, 1400, 3000, 5000, 5500};
   const int want_groups[6] = {1, 2, 3, 5, 8, 9};
   std::vector<int32_t> l65;
   b.add(10, 4);
   for (int i = 0; i < 6; ++i) {
      l65.push_back((int32_t)b.n());
      b.add(rows65[i], 65);
      if (i % 2) b.add(20 + i, 3 + i);
   }
   const int32_t l_norows = (int32_t)b.n();
   b.add(0, 70);
   b.add(300, 40);
   const int32_t l400 = (int32_t)b.n();
   b.add(200, 400);
   b.add(5, 2);
   for (int i = 0; i < 6; ++i) {
      const int layout = sb::wide_layout_for(65, rows65[i]);
      CHECK(layout >= 0 && (rows65[i] + sb::wide_rows_per_block(layout) - 1) / sb::wide_rows_per_block(layout) == want_groups[i]);
   }
   for (int no_wide = 0; no_wide < 2; ++no_wide) {
      sb::HostPlan plan;
      const char *err = "";
      CHECK(sb::build_host_plan(b.n(), b.row_off.data(), b.iso_off.data(), b.f_off.data(), n_cu, sb::PlanTuning(), &plan, &err) == 0);
      sb::SizeClass *stream = nullptr;
      for (sb::SizeClass &sc : plan.classes)
         if (sc.kind == sb::kStream) {
            CHECK(!stream); // one streaming class
            stream = &sc;
         }
      CHECK(stream);
      const std::vector<int32_t> before = stream->loci;
      CHECK(before.size() == 8); // the six of 65 isoforms, the one without rows, the one of 400
      const sb::WidePacking w = sb::pack_wide_rounds(&plan, b.row_off.data(), b.iso_off.data(), n_cu, no_wide != 0);
      if (no_wide) {
         CHECK(w.rounds.empty() && w.table.empty() && w.buf_doubles == 0 && w.n_wide_loci == 0);
         CHECK(stream->loci == before && stream->n_blocks == 8);
         continue;
      }
      // ---- first fit, most workgroups first, stable: restated
      struct Item {
         int32_t locus;
         int64_t G;
      };
      std::vector<Item> items;
      std::vector<int32_t> rest;
      for (int32_t l : before) {
         const int layout = sb::wide_layout_for(b.niso(l), b.nrow(l));
         const int64_t G = layout < 0 ? 0 : (b.nrow(l) + sb::wide_rows_per_block(layout) - 1) / sb::wide_rows_per_block(layout);
         if (G >= 1 && G <= n_cu) items.push_back({l, G});
         else rest.push_back(l);
      }
      CHECK(rest.size() == 2 && std::count(rest.begin(), rest.end(), l65[5]) == 1 && std::count(rest.begin(), rest.end(), l_norows) == 1);
      std::vector<size_t> order(items.size());
      std::iota(order.begin(), order.end(), (size_t)0);
      for (size_t i = 1; i < order.size(); ++i) // (an insertion sort keeps equal keys in input order)
         for (size_t j = i; j > 0 && items[order[j - 1]].G < items[order[j]].G; --j) std::swap(order[j - 1], order[j]);
      std::vector<std::vector<Item>> bins;
      for (size_t o : order) {
         size_t r = 0;
         for (; r < bins.size(); ++r) {
            int64_t used = 0;
            for (const Item &it : bins[r]) used += it.G;
            if (used + items[o].G <= n_cu) break;
         }
         if (r == bins.size()) bins.emplace_back();
         bins[r].push_back(items[o]);
      }
      // 8 | 5 3 | 2 1 + the 400-isoform locus' 2: three rounds
      CHECK(bins.size() == 3 && w.rounds.size() == bins.size());
      size_t at = 0;
      int64_t buf = 0;
      std::vector<int32_t> table_loci;
      for (size_t r = 0; r < bins.size(); ++r) {
         const sb::WideRound &round = w.rounds[r];
         CHECK(round.first_desc == (int)at && round.n_desc == (int)bins[r].size() && round.n_blocks <= n_cu);
         int32_t first_block = 0;
         size_t lds = 0;
         for (const Item &it : bins[r]) {
            CHECK(at < w.table.size());
            const sb::WideDesc &d = w.table[at++];
            const int64_t nrow = b.nrow(it.locus);
            CHECK(d.locus == it.locus && d.n_blocks == it.G && d.first_block == first_block);
            CHECK(d.rows_per_block == (nrow + it.G - 1) / it.G && (int64_t)d.rows_per_block * d.n_blocks >= nrow);
            CHECK(d.layout == sb::wide_layout_for(b.niso(it.locus), nrow) && d.npad == sb::wide_cols(d.layout) && d.npad >= b.niso(it.locus));
            CHECK(d.rows_per_block <= sb::wide_rows_per_block(d.layout));
            CHECK(d.buf_off == buf && d.pad_ == 0);
            // the slice: the smallest power of two of columns that, times G, covers the padded width
            CHECK(((int64_t)it.G << d.lb_slice) >= d.npad && (d.lb_slice == 0 || ((int64_t)it.G << (d.lb_slice - 1)) < d.npad));
            buf += 4 * it.G * d.npad + 4 * d.npad;
            first_block += (int32_t)it.G;
            lds = std::max(lds, sb::wide_lds_bytes(d.layout));
            table_loci.push_back(it.locus);
         }
         CHECK(round.n_blocks == first_block && round.lds_bytes == lds);
      }
      CHECK(at == w.table.size() && w.buf_doubles == (size_t)buf);
      CHECK(w.table[0].locus == l65[4] && w.table[0].n_blocks == 8 && w.table[1].locus == l65[3] && w.table[2].locus == l65[2]);
      CHECK(std::count(table_loci.begin(), table_loci.end(), l400) == 1);
      // the class list: the table's loci, then the rest as it was; the streaming kernel keeps the rest
      std::vector<int32_t> list = table_loci;
      list.insert(list.end(), rest.begin(), rest.end());
      CHECK(stream->loci == list && w.n_wide_loci == 6 && stream->n_blocks == 2);

      // ---- the head of the arena as staged: tables, class sizes, lists, the wide table, the offsets
      const sb::PlanLayout L = sb::plan_arena_layout(plan, w.table.size(), w.buf_doubles);
      std::vector<char> head(L.staged, 0);
      const sb::PlanHead h = sb::stage_plan_head(plan, L, b.row_off.data(), b.iso_off.data(), b.f_off.data(), w.table, head.data());
      CHECK(std::memcmp(head.data() + L.row_off, b.row_off.data(), b.row_off.size() * 8) == 0);
      CHECK(std::memcmp(head.data() + L.iso_off, b.iso_off.data(), b.iso_off.size() * 8) == 0);
      CHECK(std::memcmp(head.data() + L.f_off, b.f_off.data(), b.f_off.size() * 8) == 0);
      CHECK(std::memcmp(head.data() + L.wide_table, w.table.data(), w.table.size() * sizeof(sb::WideDesc)) == 0);
      const sb::ClassRecord *table = (const sb::ClassRecord *)(head.data() + L.tables);
      const int32_t *class_n = (const int32_t *)(head.data() + L.class_n), *lists = (const int32_t *)(head.data() + L.loci);
      int32_t off = 0;
      int blocks[sb::kNumKinds] = {}, classes[sb::kNumKinds] = {};
      CHECK(h.loci_off.size() == plan.classes.size());
      for (size_t ci = 0; ci < plan.classes.size(); ++ci) {
         const sb::SizeClass &sc = plan.classes[ci];
         const sb::KindLaunch &kl = h.launches[sc.kind];
         CHECK(table[ci].n == (int32_t)sc.loci.size() && class_n[ci] == table[ci].n && table[ci].loci_off == off && h.loci_off[ci] == off);
         CHECK(table[ci].block_begin == blocks[sc.kind] && table[ci].shape == (sc.layout | (sc.rmult << 8) | (sc.lbG << 16)));
         CHECK((int)ci >= kl.first_class && (int)ci < kl.first_class + kl.n_classes);
         if (classes[sc.kind] == 0) CHECK(kl.first_class == (int)ci && kl.block_threads == sc.block_threads);
         CHECK(sc.loci.empty() || std::memcmp(lists + off, sc.loci.data(), sc.loci.size() * 4) == 0);
         blocks[sc.kind] += sc.n_blocks, classes[sc.kind] += 1, off += (int32_t)sc.loci.size();
      }
      CHECK(off == b.n());
      for (int k = 0; k < sb::kNumKinds; ++k) CHECK(h.launches[k].n_blocks == blocks[k] && h.launches[k].n_classes == classes[k]);
      CHECK(h.launches[sb::kStream].n_blocks == 2 && h.max_stream_iso == 400);
      CHECK(*(const unsigned *)(head.data() + L.epi_ticket) == 0);
   }
   return 0;
}

static int layout()
{
   static_assert(sizeof(sb::ClassRecord) == 16 && sizeof(sb::WideDesc) == 40, "the kernels read 16-byte class records and 40-byte wide descriptors");
   sb::HostPlan plan;
   plan.n_loci = 40, plan.n_rows = 300;
   plan.classes.resize(3);
   // ---- one phase: nothing to zero
   {
      const sb::PlanLayout L = sb::plan_arena_layout(plan, 5, 1000);
      CHECK(L.lat.empty() && L.zero_bytes == 0 && L.staged == L.zero);
      CHECK(L.row_off == 0 && L.iso_off == 512 && L.f_off == 1024 && L.loci == 1536 && L.tables == 1792 && L.class_n == 2048 && L.wide_table == 2304);
      CHECK(L.epi_ticket == 2560 && L.staged == 2816 && L.row_keep == 2816 && L.locus_sum == 3328 && L.wide_bufs == 3840 && L.bytes == 3840 + up(1001 * 8));
      CHECK(laid_out({L.row_off, L.iso_off, L.f_off, L.loci, L.tables, L.class_n, L.wide_table, L.epi_ticket, L.row_keep, L.locus_sum, L.wide_bufs},
                     {41 * 8, 41 * 8, 41 * 8, 41 * 4, 4 * 16, 4 * 4, 6 * 40, 4, 301, 41 * 8, 1001 * 8}, L.bytes));
      // an empty batch still gives every array one element
      const sb::PlanLayout E = sb::plan_arena_layout(sb::HostPlan(), 0, 0);
      CHECK(E.bytes == 11 * 256 && E.staged == 8 * 256 && E.zero_bytes == 0);
   }
   // ---- two later phases of 70 and 300 classes (their counts: one and five granules of 256 bytes); 12 loci can reach them
   {
      plan.lat.resize(2);
      plan.lat[0].classes.resize(70), plan.lat[0].capacity.assign(70, 0), plan.lat[0].capacity[0] = 5, plan.lat[0].capacity[69] = 7;
      plan.lat[1].classes.resize(300), plan.lat[1].capacity.assign(300, 0), plan.lat[1].capacity[3] = 4;
      const sb::PlanLayout L = sb::plan_arena_layout(plan, 0, 0);
      CHECK(L.lat.size() == 2);
      std::vector<size_t> off = {L.row_off, L.iso_off, L.f_off, L.loci, L.tables, L.class_n, L.wide_table,
                                 L.lat[0].table, L.lat[0].route, L.lat[1].table, L.lat[1].route, L.epi_ticket,
                                 L.lat[0].counts, L.lat[0].total, L.lat[1].counts, L.lat[1].total,
                                 L.lat[0].lists, L.lat[1].lists, L.row_keep, L.locus_sum, L.wide_bufs};
      std::vector<size_t> bytes = {41 * 8, 41 * 8, 41 * 8, 41 * 4, 4 * 16, 4 * 4, 1 * 40,
                                   71 * 16, 41 * 4, 301 * 16, 41 * 4, 4,
                                   71 * 4, 4, 301 * 4, 4,
                                   13 * 4, 13 * 4, 301, 41 * 8, 8};
      CHECK(laid_out(off, bytes, L.bytes));
      // the staged head ends where the zeroed region begins, and that region is exactly the phases' counts and totals
      CHECK(L.staged == L.epi_ticket + 256 && L.staged <= L.zero && L.zero == L.lat[0].counts);
      CHECK(L.zero_bytes == up(71 * 4) + 256 + up(301 * 4) + 256 && L.zero + L.zero_bytes == L.lat[0].lists);
      for (size_t i = 0; i < off.size(); ++i) CHECK((off[i] < L.staged) == (i < 12));
   }
   return 0;
}

int main()
{
   if (packing() || layout()) return 1;
   std::printf("ok\n");
   return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_wide_cpp")
    src, exe = d / "plan_wide.cpp", d / "plan_wide"
    src.write_text(PROGRAM)
    csrc = os.path.join(ROOT, "strawberry_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-I", csrc, str(src), os.path.join(csrc, "plan.cpp"), "-o", str(exe)])
    return exe


def test_wide_rounds_arena_layout_and_staged_head_match_their_restatements(program):
    out = subprocess.run([str(program)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
