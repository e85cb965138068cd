// The trace of one input as one row of int64 words: what run_model computes and the prover reads, flattened by a layout that the host
// (trace_to_row) and the device inference (infer.h: the taps of infer_plan, k_infer_tap_pack) share. A row is described by entries
// (node, role, offset, len) in node order; within a node: for an Mha node role TRACE_ROLE_MHA_IN (the products Q K^T its Softmax reads) and then
// TRACE_ROLE_MHA_OUT (the probabilities), then roles 0, 1, 2 for the node's output slots (QKV has three). A Flatten node's output is entered
// like any other (a copy of its input). NOT in the row: the model inputs (the caller has them) and everything derived — the FFT tables of a
// Conv node and the row maxima of a Logits node, which trace_from_row makes again from the tapped tensors.
#pragma once
#include "zkml.h"

namespace dp {

constexpr uint64_t TRACE_ROLE_MHA_IN = 16, TRACE_ROLE_MHA_OUT = 17;
struct TraceEntry { uint64_t node, role, off, len; };
struct TraceLayout {
  std::vector<TraceEntry> entries; size_t row_words = 0;
  std::vector<size_t> first;  // first[id]: the entry of output slot 0 of node id (its other slots follow it, an Mha node's two inner tensors precede it)
};
inline TraceLayout trace_layout(const ModelSpec& m) {
  TraceLayout t;
  std::vector<size_t> lens; tensor_lens(m, lens);
  auto add = [&](size_t id, uint64_t role, size_t len) { t.entries.push_back(TraceEntry{(uint64_t)id, role, (uint64_t)t.row_words, (uint64_t)len}); t.row_words += len; };
  t.first.resize(m.layers.size());
  for (size_t id = 0; id < m.layers.size(); id++) {
    const LayerSpec& l = m.layers[id];
    if (l.kind == L_MHA) { const size_t n = l.mha_shape[1] * l.mha_shape[0] * l.mha_shape[0]; add(id, TRACE_ROLE_MHA_IN, n); add(id, TRACE_ROLE_MHA_OUT, n); }
    t.first[id] = t.entries.size();
    for (size_t s = 0; s < out_degree(l); s++) add(id, s, lens[id]);
  }
  return t;
}
// row: lay.row_words words. Throws DP_ERR_SHAPE when a tensor of the trace has not the length the layout gives it
inline void trace_to_row(const ModelSpec& m, const TraceLayout& lay, const Trace& tr, int64_t* row) {
  for (const TraceEntry& e : lay.entries) {
    const size_t id = (size_t)e.node;
    const std::vector<int64_t>* v;
    if (e.role == TRACE_ROLE_MHA_IN || e.role == TRACE_ROLE_MHA_OUT) {
      auto it = tr.mha.find(id);
      DP_REQUIRE(it != tr.mha.end() && m.layers[id].kind == L_MHA, DP_ERR_SHAPE, "trace row: no Mha data for the node");
      v = e.role == TRACE_ROLE_MHA_IN ? &it->second.softmax_in : &it->second.softmax_out;
    } else v = &tr.tensor((int)id, (int)e.role);
    DP_REQUIRE(v->size() == e.len, DP_ERR_SHAPE, "trace row: tensor length");
    std::copy(v->begin(), v->end(), row + e.off);
  }
}
// The Trace of run_model(m, input), every field prove() and witness_host read, from the input and its row: in / in2 / in3 follow the edges, out /
// more_out / mha are the row's slices, argmax_max[id][r] = in[id][r K + out[id][r]], and conv[id] comes from conv_op on the tapped input — the FFT
// tables are witness and stay host work; the node's output is then what conv_op returns (which equals the tap: the device convolves the same integers)
inline Trace trace_from_row(const ModelSpec& m, const TraceLayout& lay, const int64_t* input, const int64_t* row) {
  Trace tr;
  const size_t n = m.layers.size();
  const std::vector<size_t> in_lens = input_tensor_lens(m);
  auto slice = [&](const TraceEntry& e) { return std::vector<int64_t>(row + e.off, row + e.off + e.len); };
  auto fetch = [&](const Edge& e) -> std::vector<int64_t> {
    if (e.from >= 0) { DP_REQUIRE((size_t)e.from < tr.out.size(), DP_ERR_SHAPE, "model graph: an edge must come from an earlier node"); return tr.tensor(e.from, e.slot); }
    size_t off = 0; for (int q = 0; q < e.slot; q++) off += in_lens.at((size_t)q);
    DP_REQUIRE((size_t)e.slot < in_lens.size() && off + in_lens[(size_t)e.slot] <= m.input_len, DP_ERR_SHAPE, "model graph: input tensor");
    return std::vector<int64_t>(input + off, input + off + in_lens[(size_t)e.slot]);
  };
  tr.in2.resize(n); tr.in3.resize(n); tr.more_out.resize(n);
  for (size_t id = 0; id < n; id++) {
    const LayerSpec& l = m.layers[id];
    const std::vector<Edge> edges = edges_in(m, id);
    DP_REQUIRE(edges.size() == in_degree(l), DP_ERR_SHAPE, "model graph: wrong number of inputs for a node");
    tr.in.push_back(fetch(edges[0]));
    if (edges.size() > 1) tr.in2[id] = fetch(edges[1]);
    if (edges.size() > 2) tr.in3[id] = fetch(edges[2]);
    const size_t f = lay.first[id];
    if (l.kind == L_MHA) { MhaTrace d; d.softmax_in = slice(lay.entries[f - 2]); d.softmax_out = slice(lay.entries[f - 1]); tr.mha[id] = std::move(d); }
    if (l.kind == L_CONV) { tr.conv.resize(n); tr.out.push_back(conv_op(l, tr.in[id], tr.conv[id])); }
    else tr.out.push_back(slice(lay.entries[f]));
    for (size_t s = 1; s < out_degree(l); s++) tr.more_out[id].push_back(slice(lay.entries[f + s]));
    if (l.kind == L_LOGITS) {
      const std::vector<int64_t>& x = tr.in[id]; const std::vector<int64_t>& idx = tr.out[id];
      DP_REQUIRE(l.nrows && l.ncols && x.size() == l.nrows * l.ncols && idx.size() == l.nrows, DP_ERR_SHAPE, "logits: input shape");
      std::vector<int64_t>& mx = tr.argmax_max[id];
      mx.resize(l.nrows);
      for (size_t r = 0; r < l.nrows; r++) { DP_REQUIRE(idx[r] >= 0 && (size_t)idx[r] < l.ncols, DP_ERR_SHAPE, "trace row: an argmax index outside its row"); mx[r] = x[r * l.ncols + (size_t)idx[r]]; }
    }
  }
  return tr;
}
inline Trace trace_from_row(const ModelSpec& m, const int64_t* input, const int64_t* row) { return trace_from_row(m, trace_layout(m), input, row); }

}  // namespace dp
