// C entry points over the row-segment plan of the Farneback row-stream kernel for every box half-width it is built for
// (denseflow_amd/csrc/farneback_plan.h), for tests/test_farn_stream_plan_cpu.py.
#include "../denseflow_amd/csrc/farneback_plan.h"

extern "C" {
int fsp_seg_rows(int w, int h, int n_pairs, int half) { return farn_stream_seg_rows(w, h, n_pairs, half); }
int fsp_seg_rows_default(int w, int h, int n_pairs) { return farn_stream_seg_rows(w, h, n_pairs); }
int fsp_min_seg_rows(int half) { return farn_stream_min_seg_rows(half); }
int fsp_has_half(int half) { return farn_stream_has_half(half) ? 1 : 0; }
int fsp_step_rows() { return kFarnStreamStepRows; }
}
