// CSV parsing on the device (readers/gpu_csv.py; the reference's default readers are CSV: CSVReaders.scala:54-122,
// DataReader.scala:173-197). The host only moves raw bytes: file chunks are read into pinned buffers and copied to
// the device, where
//   csv_fields_kernel   one wave per row walks the row in 64-byte windows (coalesced loads), finds the separators
//                       outside double quotes with two ballots (the quote parity of each lane is the popcount of
//                       the quotes below it) and writes every field's start offset; a row that ends inside quotes
//                       (a newline in a quoted field) is reported with nfields = -1;
//   csv_parse_num       one thread per (row, column): the field as a float64 or int64 with a validity byte --
//                       pandas' NA strings and empty cells are missing; decimal strings of at most 19 significant
//                       digits with |exponent| <= 22 convert exactly (one IEEE multiply or divide of two exact
//                       doubles: the correctly rounded result), anything else is flagged for the host parser;
//   csv_hash_text       one thread per (row, column): a 64-bit hash of the decoded field bytes (0 = missing), the
//                       input of the device dictionary encoding (stable sort + first appearance), and a second,
//                       independent hash that tells two strings with one first hash apart.
// A cell's value follows pyarrow's CSV reader: a field whose first and last raw bytes are double quotes is quoted
// (the quotes go, "" inside is one quote); any other field is literal, padding and quotes included. Numbers are
// parsed from the value with spaces and tabs trimmed; the NA strings are compared with the untrimmed value.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip/tmog_hip_abi.h"

namespace {

__device__ __forceinline__ uint64_t lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// buf: the chunk's bytes; row_start[r] .. row_end[r] (exclusive, the '\n' or the chunk end) are row r's bytes (a
// trailing '\r' is dropped). fstart[r * (ncols + 1) + k] = absolute offset of field k, fstart[.. + nf] = end + 1 (so
// field k is [fstart[k], fstart[k + 1] - 1)); nfields[r] = number of fields (fields past ncols are not recorded), or
// -1 when the row ends inside quotes: its newline belongs to a quoted field, which this reader does not parse.
__global__ void __launch_bounds__(256) csv_fields_kernel(const uint8_t* __restrict__ buf,
                                                         const int64_t* __restrict__ row_start,
                                                         const int64_t* __restrict__ row_end, int64_t nrows,
                                                         int ncols, int sep, int64_t* __restrict__ fstart,
                                                         int32_t* __restrict__ nfields) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= nrows) return;
  const int64_t b0 = row_start[r];
  int64_t e = row_end[r];
  if (e > b0 && buf[e - 1] == '\r') --e;
  int64_t* fs = fstart + r * (int64_t)(ncols + 1);
  if (lane == 0) fs[0] = b0;
  int nf = 1;                   // fields so far (wave-uniform)
  int quote = 0;                // quote parity carried from the previous windows
  for (int64_t p = b0; p < e; p += 64) {
    const int64_t q = p + lane;
    const uint8_t c = q < e ? buf[q] : 0;
    const uint64_t qm = __ballot(c == '"');
    const int inq = (quote + __popcll(qm & lanes_below(lane))) & 1;
    const bool is_sep = c == (uint8_t)sep && !inq && q < e;
    const uint64_t sm = __ballot(is_sep);
    if (is_sep) {
      const int k = nf + __popcll(sm & lanes_below(lane));
      if (k <= ncols - 1) fs[k] = q + 1;
    }
    nf += __popcll(sm);
    quote = (quote + __popcll(qm)) & 1;
  }
  if (lane == 0) {
    fs[min(nf, ncols)] = e + 1;
    nfields[r] = quote ? -1 : nf;
  }
}

__device__ __forceinline__ bool is_space(uint8_t c) { return c == ' ' || c == '\t'; }

// pandas.read_csv's default NA strings (readers/columnar.py _PANDAS_NA), compared with the cell's value
// (unquoted, not trimmed)
__device__ bool is_na(const uint8_t* s, int n) {
  if (n == 0) return true;
  if (n > 8) return false;
  const uint8_t c0 = s[0];              // every NA string starts with one of these
  if (!(c0 == '#' || c0 == '-' || c0 == '1' || c0 == '<' || c0 == 'N' || c0 == 'n')) return false;
  char t[9];
  for (int i = 0; i < n; ++i) t[i] = (char)s[i];
  t[n] = 0;
  const char* na[] = {"#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>",
                      "N/A", "NA", "NULL", "NaN", "None", "n/a", "nan", "null"};
  for (int k = 0; k < 18; ++k) {
    const char* a = na[k];
    int i = 0;
    while (i < n && a[i] && a[i] == t[i]) ++i;
    if (i == n && a[i] == 0) return true;
  }
  return false;
}

// the value of field col of a row: its raw bytes, without the quotes when the first and the last byte are quotes
// (*quoted: "" inside is an escape); an absent field (col >= nf, or a row reported as -1) is empty
__device__ __forceinline__ void field_value(const uint8_t* buf, const int64_t* fs, int nf, int col, int64_t* a,
                                            int64_t* b, bool* quoted) {
  *quoted = false;
  if (col >= nf) {
    *a = *b = 0;
    return;
  }
  int64_t s = fs[col], t = fs[col + 1] - 1;
  if (t - s >= 2 && buf[s] == '"' && buf[t - 1] == '"') {
    ++s;
    --t;
    *quoted = true;
  }
  *a = s;
  *b = t;
}

__constant__ double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                  1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// One (row, column) per thread, row-major: the threads of a wave read one row's consecutive field offsets and bytes.
// cols[j] = CSV column of output j; kind[j] = 0 float64, 1 int64. out[r * nout + j] (as double or int64 bits),
// valid[r * nout + j]; slow[r * nout + j] = 1 when the host must parse the field (the host transposes the tile to
// column-major). A field that does not parse as a number is checked against the NA strings only then.
__global__ void __launch_bounds__(256) csv_parse_num_kernel(const uint8_t* __restrict__ buf,
                                                            const int64_t* __restrict__ fstart,
                                                            const int32_t* __restrict__ nfields, int64_t nrows,
                                                            int ncols, const int32_t* __restrict__ cols,
                                                            const int32_t* __restrict__ kind, int nout,
                                                            int64_t* __restrict__ out, uint8_t* __restrict__ valid,
                                                            uint8_t* __restrict__ slow) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows * nout) return;
  const int64_t r = i / nout;
  const int j = (int)(i - r * nout);
  const int64_t o = i;
  int64_t a, b;
  bool quoted;
  field_value(buf, fstart + r * (int64_t)(ncols + 1), nfields[r], cols[j], &a, &b, &quoted);
  const int64_t ua = a, ub = b;         // the untrimmed value: what the NA strings are compared with
  slow[o] = 0;
  valid[o] = 0;
  out[o] = 0;
  if (a == b) return;                   // an empty cell (or ""): missing
  while (a < b && is_space(buf[a])) ++a;
  while (b > a && is_space(buf[b - 1])) --b;
  const uint8_t* s = buf + a;
  const int n = (int)(b - a);
  if (n == 0) {                         // only padding: not a number and not NA, the host rejects it
    slow[o] = 1;
    return;
  }
  int k = 0;
  bool neg = false, plus = false;
  if (s[k] == '+' || s[k] == '-') {
    neg = s[k] == '-';
    plus = s[k++] == '+';
  }
  uint64_t m = 0;
  int nd = 0, e10 = 0;
  bool any = false, dot = false, bad = false, hasexp = false;
  for (; k < n; ++k) {
    const uint8_t c = s[k];
    if (c >= '0' && c <= '9') {
      any = true;
      if (m == 0 && c == '0') {         // leading zeros do not count as significant digits
        if (dot) --e10;
        continue;
      }
      if (nd < 19) {
        m = m * 10 + (c - '0');
        ++nd;
        if (dot) --e10;
      } else {
        bad = bad || c != '0';          // a 20th significant digit that matters: host
        if (!dot) ++e10;
      }
    } else if (c == '.' && !dot) {
      dot = true;
    } else {
      break;
    }
  }
  if (k < n && (s[k] == 'e' || s[k] == 'E') && any) {
    ++k;
    hasexp = true;
    bool eneg = false;
    if (k < n && (s[k] == '+' || s[k] == '-')) eneg = s[k++] == '-';
    int ev = 0;
    bool edig = false;
    for (; k < n && s[k] >= '0' && s[k] <= '9'; ++k) {
      edig = true;
      ev = min(ev * 10 + (s[k] - '0'), 100000);
    }
    bad = bad || !edig;
    e10 += eneg ? -ev : ev;
  }
  if (!any || k != n) {                 // not a plain decimal: an NA string is missing, anything else (inf,
    if (is_na(buf + ua, (int)min(ub - ua, (int64_t)9))) return;       // hex, stray characters) goes to the host
    bad = true;
  }
  if (kind[j] == 1) {                   // int64: plain [-]digits; '+', a fraction (".0" too) or an exponent: host
    if (bad || plus || dot || hasexp || nd > 18) {
      slow[o] = 1;
      return;
    }
    out[o] = neg ? -(int64_t)m : (int64_t)m;
    valid[o] = 1;
    return;
  }
  double v;
  if (!bad && m == 0) {
    v = 0.0;
  } else if (!bad && m < (1ull << 53) && e10 >= -22 && e10 <= 22) {
    const double dm = (double)m;        // exact
    v = e10 >= 0 ? dm * kPow10[e10] : dm / kPow10[-e10];     // one correctly rounded IEEE operation
  } else {
    slow[o] = 1;
    return;
  }
  v = neg ? -v : v;
  out[o] = __double_as_longlong(v);
  valid[o] = 1;
}

// hash[o]: 64-bit FNV-1a of the cell's decoded bytes (a quoted field without its quotes, "" as one quote; any other
// field as written), 0 for a missing cell (an NA string or empty). check[o]: a second hash of the same bytes with
// another mixing function and the length folded in (0 for missing): cells of one hash[] value with different check[]
// values are different strings. span[o] = the field's raw byte range, quotes included (the host decodes the
// vocabulary from it by the same rule); (-1, -1) for a field that starts with a quote and is not a well-formed
// quoted field (text after the closing quote, a single quote inside), which this reader does not parse.
__global__ void __launch_bounds__(256) csv_hash_text_kernel(const uint8_t* __restrict__ buf,
                                                            const int64_t* __restrict__ fstart,
                                                            const int32_t* __restrict__ nfields, int64_t nrows,
                                                            int ncols, const int32_t* __restrict__ cols, int nout,
                                                            uint64_t* __restrict__ hash, int64_t* __restrict__ span,
                                                            uint64_t* __restrict__ check) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows * nout) return;
  const int64_t r = i / nout;           // row-major as csv_parse_num: out[r * nout + j]
  const int j = (int)(i - r * nout);
  const int64_t o = i;
  int64_t a, b;
  bool quoted;
  field_value(buf, fstart + r * (int64_t)(ncols + 1), nfields[r], cols[j], &a, &b, &quoted);
  span[2 * o] = quoted ? a - 1 : a;
  span[2 * o + 1] = quoted ? b + 1 : b;
  hash[o] = 0;
  check[o] = 0;
  if (is_na(buf + a, (int)min(b - a, (int64_t)9))) return;
  bool odd = !quoted && buf[a] == '"';  // an opening quote without its closing quote at the field's end
  uint64_t h = 14695981039346656037ull, g = 0x9E3779B97F4A7C15ull;
  int64_t len = 0;
  for (int64_t p = a; p < b; ++p, ++len) {
    const uint8_t c = buf[p];
    if (quoted && c == '"') {           // "" is one quote; a single quote inside a quoted field is not parsed
      if (p + 1 < b && buf[p + 1] == '"') ++p;
      else odd = true;
    }
    h ^= c;
    h *= 1099511628211ull;
    g = (g ^ c) * 0xFF51AFD7ED558CCDull;
    g ^= g >> 32;
  }
  if (odd) {
    span[2 * o] = span[2 * o + 1] = -1;
    return;
  }
  hash[o] = h ? h : 1;                  // 0 is reserved for missing
  check[o] = g ^ (uint64_t)len;
}

}  // namespace

extern "C" {

int tmog_hip_csv_fields(const uint8_t* buf, const int64_t* row_start, const int64_t* row_end, int64_t nrows,
                        int ncols, int sep, int64_t* fstart, int32_t* nfields, hipStream_t stream) {
  if (nrows <= 0) return 0;
  if (ncols < 1) return -2;
  const int64_t blocks = (nrows + 3) / 4;   // 4 waves (rows) per workgroup
  hipLaunchKernelGGL(csv_fields_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, buf, row_start, row_end, nrows,
                     ncols, sep, fstart, nfields);
  return (int)hipGetLastError();
}

int tmog_hip_csv_parse_num(const uint8_t* buf, const int64_t* fstart, const int32_t* nfields, int64_t nrows, int ncols,
                           const int32_t* cols, const int32_t* kind, int nout, int64_t* out, uint8_t* valid,
                           uint8_t* slow, hipStream_t stream) {
  const int64_t n = nrows * (int64_t)nout;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(csv_parse_num_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, buf, fstart,
                     nfields, nrows, ncols, cols, kind, nout, out, valid, slow);
  return (int)hipGetLastError();
}

int tmog_hip_csv_hash_text(const uint8_t* buf, const int64_t* fstart, const int32_t* nfields, int64_t nrows,
                           int ncols, const int32_t* cols, int nout, uint64_t* hash, int64_t* span,
                           uint64_t* check, hipStream_t stream) {
  const int64_t n = nrows * (int64_t)nout;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(csv_hash_text_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, buf, fstart,
                     nfields, nrows, ncols, cols, nout, hash, span, check);
  return (int)hipGetLastError();
}

}  // extern "C"
