// Structure files on the device: PDB text -> the library's receptor arrays (kpd_pdb_parse) and SDF / MOL V2000 text -> the layout of
// kpd_mol_perceive (kpd_sdf_parse), for a batch of files in one byte buffer; include/kpd.h is the definition of both.  The inverse
// of the text writers of emit.hip / molecule.hip.  Replaces the parsing that upstream leaves to prody / BioPython / RDKit (byop.py,
// process_crossdocked.py, process_bindingmoad.py, parse_ligand).
// Both begin alike: line starts counted per tile of the concatenated buffer, one exclusive scan, line starts written and classified.
// PDB (six launches whatever B is): kept records counted per file, one scan, records parsed, a thread per record.  SDF (ten launches
// and a memset): records counted per file, one scan, their line ranges, then one wave per record twice: sizes (two scans) and
// outputs, the bond graph as the bit matrices of k_mol_perceive so that its steps 5-6 are shared (molecule_core.h).
// No host synchronisation.  Integer arithmetic, one IEEE fp64 division per real field, no float atomics: every output is bitwise
// independent of batch composition.  Every read of `text` is guarded by the buffer's size and every write by a capacity, so any
// bytes whatsoever end in statuses, never in a fault.
#include "common.h"
#include "engine.h"
#include "molecule_core.h"
#include "scan_core.h"

namespace kpd {

constexpr int ST_THREADS = 256;
constexpr int ST_TILE = KPD_STRUCT_TILE;        // bytes of the buffer per workgroup: one aligned 16-byte load per thread
static_assert(ST_TILE == ST_THREADS * 16, "one 16-byte load per thread");
constexpr int ST_COLS = 80;                     // columns of a line that are read

enum : int { LC_OTHER = 0, LC_ATOM = 1, LC_HETATM = 2, LC_ENDMDL = 3, LC_SEP = 4, LC_BLANK = 5 };     // 1 - 3: PDB text; 4, 5: SDF text
enum : int { PF_HETATM = 1, PF_HYDROGEN = 2, PF_WATER = 4, PF_ALTLOC = 8, PF_STD_AA = 16, PF_CALPHA = 32, PF_GUESSED = 64, PF_BAD = 128 };
enum : int { PS_EMPTY = 1, PS_CAPACITY = 2, PS_BAD_RECORD = 4, PS_MODELS = 8, PS_BAD_SEGMENT = 16, PS_LINES = 32 };

__host__ __device__ constexpr unsigned pack3(char a, char b, char c) {
    return (unsigned)(unsigned char)a | ((unsigned)(unsigned char)b << 8) | ((unsigned)(unsigned char)c << 16);
}
__host__ __device__ constexpr unsigned pack2(char a, char b) { return pack3(a, b, 0); }

// the tables of include/kpd.h
__device__ const unsigned STD_AA[20] = {pack3('A', 'L', 'A'), pack3('A', 'R', 'G'), pack3('A', 'S', 'N'), pack3('A', 'S', 'P'),
                                        pack3('C', 'Y', 'S'), pack3('G', 'L', 'N'), pack3('G', 'L', 'U'), pack3('G', 'L', 'Y'),
                                        pack3('H', 'I', 'S'), pack3('I', 'L', 'E'), pack3('L', 'E', 'U'), pack3('L', 'Y', 'S'),
                                        pack3('M', 'E', 'T'), pack3('P', 'H', 'E'), pack3('P', 'R', 'O'), pack3('S', 'E', 'R'),
                                        pack3('T', 'H', 'R'), pack3('T', 'R', 'P'), pack3('T', 'Y', 'R'), pack3('V', 'A', 'L')};
__device__ const unsigned WATERS[7] = {pack3('H', 'O', 'H'), pack3('D', 'O', 'D'), pack3('W', 'A', 'T'), pack3('H', '2', 'O'),
                                       pack3('O', 'H', '2'), pack3('T', 'I', 'P'), pack3('S', 'O', 'L')};
__device__ const unsigned TWO_LETTER[44] = {
    pack2('L', 'i'), pack2('B', 'e'), pack2('N', 'e'), pack2('N', 'a'), pack2('M', 'g'), pack2('A', 'l'), pack2('S', 'i'), pack2('C', 'l'),
    pack2('A', 'r'), pack2('C', 'a'), pack2('S', 'c'), pack2('T', 'i'), pack2('C', 'r'), pack2('M', 'n'), pack2('F', 'e'), pack2('C', 'o'),
    pack2('N', 'i'), pack2('C', 'u'), pack2('Z', 'n'), pack2('G', 'a'), pack2('G', 'e'), pack2('A', 's'), pack2('S', 'e'), pack2('B', 'r'),
    pack2('K', 'r'), pack2('R', 'b'), pack2('S', 'r'), pack2('Z', 'r'), pack2('M', 'o'), pack2('R', 'u'), pack2('R', 'h'), pack2('P', 'd'),
    pack2('A', 'g'), pack2('C', 'd'), pack2('I', 'n'), pack2('S', 'n'), pack2('S', 'b'), pack2('T', 'e'), pack2('X', 'e'), pack2('C', 's'),
    pack2('B', 'a'), pack2('P', 't'), pack2('A', 'u'), pack2('P', 'b')};
__device__ const double POW10[16] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};

__device__ __forceinline__ long long clamp_ll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// first index in [0, n] whose entry is >= v; a ascending (any a: the answer stays in [0, n])
__device__ __forceinline__ int lower_bound_ll(const long long *__restrict__ a, int n, long long v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- line starts of one tile -------------------------------------------------------------------------------------
// Tile t covers the positions [t * ST_TILE - a0, (t + 1) * ST_TILE - a0) of the buffer, a0 = the misalignment of `text`, so that
// every thread's 16 bytes are one aligned load; the partial chunks at the two ends of the buffer are read byte by byte.
// buf: the tile's bytes behind one 16-byte slot whose last byte is the byte in front of the tile.  bnd: 1 where a file begins or ends.
// Returns the 16-bit mask of the line starts among this thread's bytes: a position of [file_ptr[0], file_ptr[B]) that is an entry
// of file_ptr or follows a '\n'.
__device__ __forceinline__ unsigned tile_line_starts(const uint8_t *__restrict__ text, long long n, const long long *__restrict__ fp, int B,
                                                     uint4 *buf, uint8_t *bnd, long long &p0) {
    const int tid = threadIdx.x;
    const long long a0 = (long long)(reinterpret_cast<uintptr_t>(text) & 15);
    const long long base = (long long)blockIdx.x * ST_TILE - a0;
    const long long lo = base < 0 ? 0 : base, hi = base + ST_TILE < n ? base + ST_TILE : n;
    p0 = base + 16 * tid;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p0 >= 0 && p0 + 16 <= n) {
        v = *reinterpret_cast<const uint4 *>(text + p0);
    } else {
        unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long long p = p0 + j;
            if (p >= 0 && p < n) w[j >> 2] |= (unsigned)text[p] << (8 * (j & 3));
        }
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    buf[1 + tid] = v;
    reinterpret_cast<uint4 *>(bnd)[tid] = make_uint4(0, 0, 0, 0);
    if (tid == 0) reinterpret_cast<uint8_t *>(buf)[15] = (base >= 1 && base - 1 < n) ? text[base - 1] : (uint8_t)0;
    __syncthreads();
    const int bf = lower_bound_ll(fp, B + 1, lo);
    for (int b = bf + tid; b <= B; b += ST_THREADS) {
        const long long q = fp[b];
        if (q < lo || q >= hi) break;
        bnd[q - base] = 1;
    }
    __syncthreads();
    const long long f0 = clamp_ll(fp[0], 0, n), fB = clamp_ll(fp[B], 0, n);
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(buf) + 15;     // bytes[i] = the byte in front of tile position i
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const long long p = p0 + j;
        const int i = 16 * tid + j;
        if (p >= lo && p < hi && p >= f0 && p < fB && (bnd[i] || bytes[i] == '\n')) mask |= 1u << j;
    }
    return mask;
}

__global__ void __launch_bounds__(ST_THREADS)
k_struct_count(const uint8_t *__restrict__ text, long long n, const long long *__restrict__ fp, int B, int *__restrict__ tile_cnt) {
    __shared__ uint4 buf[ST_THREADS + 1];
    __shared__ __attribute__((aligned(16))) uint8_t bnd[ST_TILE];
    __shared__ int part[ST_THREADS / 64];
    long long p0;
    const unsigned mask = tile_line_starts(text, n, fp, B, buf, bnd, p0);
    int total;
    block_exclusive<ST_THREADS>((int)__popc(mask), part, total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// the file of position p (file_ptr[b] <= p < file_ptr[b + 1]), or -1
__device__ __forceinline__ int file_of(const long long *__restrict__ fp, int B, long long p) {
    const int b = lower_bound_ll(fp, B + 1, p + 1) - 1;         // the last entry <= p
    return (b >= 0 && b < B && fp[b] <= p && p < fp[b + 1]) ? b : -1;
}

__global__ void __launch_bounds__(ST_THREADS)
k_struct_lines(const uint8_t *__restrict__ text, long long n, const long long *__restrict__ fp, int B, const int *__restrict__ tile_ptr,
               int cap_lines, int sdf, long long *__restrict__ line_start, uint8_t *__restrict__ line_class) {
    __shared__ uint4 buf[ST_THREADS + 1];
    __shared__ __attribute__((aligned(16))) uint8_t bnd[ST_TILE];
    __shared__ int part[ST_THREADS / 64];
    long long p0;
    unsigned mask = tile_line_starts(text, n, fp, B, buf, bnd, p0);
    int total;
    int k = tile_ptr[blockIdx.x] + block_exclusive<ST_THREADS>((int)__popc(mask), part, total);
    for (; mask; mask &= mask - 1, ++k) {
        if (k < 0 || k >= cap_lines) continue;
        const long long p = p0 + (__ffs(mask) - 1);
        int cls = LC_OTHER;
        const int b = file_of(fp, B, p);
        const long long fend = b >= 0 ? clamp_ll(fp[b + 1], 0, n) : 0;
        if (sdf) {                                              // "$$$$", or a line without content
            if (b >= 0 && p + 4 <= fend && text[p] == '$' && text[p + 1] == '$' && text[p + 2] == '$' && text[p + 3] == '$') cls = LC_SEP;
            else if (b >= 0 && (text[p] == '\n' || (text[p] == '\r' && (p + 1 == fend || text[p + 1] == '\n')))) cls = LC_BLANK;
        } else if (b >= 0 && p + 6 <= fend) {                   // six bytes of this file; the patterns hold no '\n'
            const unsigned w0 = text[p] | (text[p + 1] << 8) | (text[p + 2] << 16) | ((unsigned)text[p + 3] << 24);
            const unsigned w1 = text[p + 4] | (text[p + 5] << 8);
            if (w0 == 0x4d4f5441u && w1 == 0x2020u) cls = LC_ATOM;              // "ATOM  "
            else if (w0 == 0x41544548u && w1 == 0x4d54u) cls = LC_HETATM;       // "HETATM"
            else if (w0 == 0x4d444e45u && w1 == 0x4c44u) cls = LC_ENDMDL;       // "ENDMDL"
        }
        line_start[k] = p;
        line_class[k] = (uint8_t)cls;
    }
}

// ---- per file: the lines of the file, its first ENDMDL, its kept records ------------------------------------------------
struct StoreTotal {
    int *out;
    __device__ void operator()(int v) const { *out = v; }
};

__global__ void __launch_bounds__(ST_THREADS)
k_pdb_count(long long n, const long long *__restrict__ fp, const int *__restrict__ n_lines_p, int cap_lines,
            const long long *__restrict__ line_start, const uint8_t *__restrict__ line_class, int *__restrict__ first_line,
            int *__restrict__ end_line, int *__restrict__ cnt, int *__restrict__ status) {
    __shared__ int part[ST_THREADS / 64];
    __shared__ int s_end;
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long f0 = fp[b], f1 = fp[b + 1];
    const int nl = *n_lines_p;
    int st = 0;
    if (f0 < 0 || f1 < f0 || f1 > n) st = PS_BAD_SEGMENT;
    else if (nl > cap_lines) st = PS_LINES;
    if (st) {
        if (tid == 0) {
            first_line[b] = end_line[b] = cnt[b] = 0;
            status[b] = st;
        }
        return;
    }
    const int l0 = lower_bound_ll(line_start, nl, f0), l1 = lower_bound_ll(line_start, nl, f1);
    if (tid == 0) s_end = l1;
    __syncthreads();
    int mine = l1;
    for (int k = l0 + tid; k < l1 && mine == l1; k += ST_THREADS)
        if (line_class[k] == LC_ENDMDL) mine = k;
    if (mine < l1) atomicMin(&s_end, mine);
    __syncthreads();
    const int le = s_end;
    int kept = 0, later = 0;
    for (int k = l0 + tid; k < l1; k += ST_THREADS) {
        const int c = line_class[k];
        const bool rec = c == LC_ATOM || c == LC_HETATM;
        kept += rec && k < le;
        later += rec && k > le;
    }
    int total, total_later;
    block_exclusive<ST_THREADS>(kept, part, total);
    block_exclusive<ST_THREADS>(later, part, total_later);
    if (tid == 0) {
        first_line[b] = l0;
        end_line[b] = le;
        cnt[b] = total;
        status[b] = (total ? 0 : PS_EMPTY) | (total_later ? PS_MODELS : 0);
    }
}

// ---- fields ------------------------------------------------------------------------------------------------------
// a line's bytes; columns beyond its end read as blanks
struct Line {
    const uint8_t *t;
    int len;
    __device__ __forceinline__ unsigned operator[](int i) const { return i < len ? (unsigned)t[i] : 0x20u; }
};

// columns [a, b) as a real: blanks, sign, digits with at most one '.', blanks; value = fp32(fp64(mantissa) / 10^k)
__device__ bool parse_real(const Line &L, int a, int b, float &out) {
    int i = a;
    while (i < b && L[i] == ' ') ++i;
    bool neg = false;
    if (i < b && (L[i] == '+' || L[i] == '-')) neg = L[i++] == '-';
    unsigned long long mant = 0;
    int digits = 0, sig = 0, k = 0;
    bool dot = false;
    for (; i < b; ++i) {
        const unsigned c = L[i];
        if (c >= '0' && c <= '9') {
            mant = mant * 10 + (c - '0');
            ++digits;
            if (mant) ++sig;
            if (dot) ++k;
            if (sig > 15 || k > 15) return false;
        } else if (c == '.' && !dot) {
            dot = true;
        } else {
            break;
        }
    }
    while (i < b && L[i] == ' ') ++i;
    if (i != b || !digits) return false;
    const double v = (double)mant / POW10[k];
    out = (float)(neg ? -v : v);
    return true;
}

// columns [a, b) as an integer: blanks, sign, digits, blanks; at most 9 digits
__device__ bool parse_int(const Line &L, int a, int b, int &out) {
    int i = a;
    while (i < b && L[i] == ' ') ++i;
    bool neg = false;
    if (i < b && (L[i] == '+' || L[i] == '-')) neg = L[i++] == '-';
    int v = 0, digits = 0;
    for (; i < b && L[i] >= '0' && L[i] <= '9'; ++i) {
        if (++digits > 9) return false;
        v = v * 10 + (int)(L[i] - '0');
    }
    while (i < b && L[i] == ' ') ++i;
    if (i != b || !digits) return false;
    out = neg ? -v : v;
    return true;
}

__device__ __forceinline__ bool is_upper(unsigned c) { return c >= 'A' && c <= 'Z'; }
__device__ __forceinline__ bool is_lower(unsigned c) { return c >= 'a' && c <= 'z'; }
__device__ __forceinline__ bool is_letter(unsigned c) { return is_upper(c) || is_lower(c); }
__device__ __forceinline__ unsigned to_upper(unsigned c) { return is_lower(c) ? c - 32 : c; }
__device__ __forceinline__ unsigned to_lower(unsigned c) { return is_upper(c) ? c + 32 : c; }

// the non-blank bytes of (c0, c1) in order, the first letter in upper and the second in lower case, packed
__device__ __forceinline__ unsigned title_symbol(unsigned c0, unsigned c1) {
    if (c0 == ' ') {
        c0 = c1;
        c1 = ' ';
    }
    if (c0 == ' ') return 0;
    return to_upper(c0) | (c1 == ' ' ? 0u : to_lower(c1) << 8);
}

template <int N>
__device__ __forceinline__ bool in_table(const unsigned (&table)[N], unsigned v) {
    bool hit = false;
#pragma unroll 4
    for (int i = 0; i < N; ++i) hit |= table[i] == v;
    return hit;
}

__device__ __forceinline__ int index_in(const unsigned *__restrict__ list, int n, unsigned v) {
    int at = n;
    for (int i = n - 1; i >= 0; --i)
        if (list[i] == v) at = i;
    return at;
}

struct PdbOut {
    float *pos, *occ_b;
    unsigned *sym;
    int *elem;
    unsigned *name, *resname;
    int *res_class, *resseq;
    unsigned *tags;
    long long *line_off;
    int *res_idx, *flags;
};

// ---- per file: parse the kept records, number the residues ----------------------------------------------------------------
__global__ void __launch_bounds__(ST_THREADS)
k_pdb_records(const uint8_t *__restrict__ text, long long n, const long long *__restrict__ fp, const int *__restrict__ n_lines_p,
              const long long *__restrict__ line_start, const uint8_t *__restrict__ line_class, const int *__restrict__ first_line,
              const int *__restrict__ end_line, const unsigned *__restrict__ symbols, int F, const unsigned *__restrict__ resnames, int R,
              const int *__restrict__ atom_ptr, int cap_atoms, PdbOut o, int *__restrict__ n_res_out, int *__restrict__ status) {
    __shared__ int part[ST_THREADS / 64];
    __shared__ unsigned keys[ST_THREADS + 1][3];         // keys[1 + r]: the residue key of the chunk's r-th kept record; keys[0]: the one before
    __shared__ int s_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (status[b] & (PS_BAD_SEGMENT | PS_LINES)) {
        if (tid == 0) n_res_out[b] = 0;
        return;
    }
    const int nl = *n_lines_p, l0 = first_line[b], le = end_line[b];
    const long long fend = fp[b + 1];                    // 0 <= fp[b] <= fend <= n: k_pdb_count checked it
    const int a0 = atom_ptr[b], a1 = atom_ptr[b + 1];
    const bool fits = a0 >= 0 && a1 >= a0 && a1 <= cap_atoms;
    if (tid == 0) s_bad = 0;
    int n_out = 0, n_res = 0;
    for (int base = l0; base < le; base += ST_THREADS) {
        const int k = base + tid;
        const int cls = k < le ? line_class[k] : LC_OTHER;
        const bool kept = cls == LC_ATOM || cls == LC_HETATM;
        int total;
        const int r = block_exclusive<ST_THREADS>((int)kept, part, total);
        // the record's fields
        float pos[3], ob[2];
        unsigned sym = 0, name = 0, resn = 0, tags = 0, key1 = 0;
        int elem = F, rclass = R, resseq = 0, flags = 0;
        long long s = 0;
        if (kept) {
            s = line_start[k];
            long long e = k + 1 < nl ? line_start[k + 1] : fend;
            e = clamp_ll(e, s, fend);
            if (e > s && text[e - 1] == '\n') --e;
            if (e > s && text[e - 1] == '\r') --e;
            const Line L{text + s, (int)(e - s < ST_COLS ? e - s : ST_COLS)};
            name = L[12] | (L[13] << 8) | (L[14] << 16) | (L[15] << 24);
            resn = L[17] | (L[18] << 8) | (L[19] << 16);
            tags = L[21] | (L[26] << 8) | (L[16] << 16);
            key1 = L[22] | (L[23] << 8) | (L[24] << 16) | (L[25] << 24);
            bool good = L.len >= 54;
            good = parse_int(L, 22, 26, resseq) && good;
            for (int c = 0; c < 3; ++c) good = parse_real(L, 30 + 8 * c, 38 + 8 * c, pos[c]) && good;
            if (!good) {
                pos[0] = pos[1] = pos[2] = __builtin_nanf("");      // resseq stays what it parsed to, or 0
                flags |= PF_BAD;
            }
            if (!parse_real(L, 54, 60, ob[0])) ob[0] = __builtin_nanf("");
            if (!parse_real(L, 60, 66, ob[1])) ob[1] = __builtin_nanf("");
            const bool std_aa = in_table(STD_AA, resn);
            if (L[76] != ' ' || L[77] != ' ') {
                sym = title_symbol(L[76], L[77]);
            } else {
                const unsigned a = L[12], c = L[13];
                if (a == ' ' || (a >= '0' && a <= '9')) sym = title_symbol(c, ' ');
                else if (is_letter(a) && std_aa) sym = title_symbol(a, ' ');
                else if (is_letter(a) && is_letter(c) && in_table(TWO_LETTER, to_upper(a) | (to_lower(c) << 8))) sym = title_symbol(a, c);
                else sym = title_symbol(a, ' ');
                flags |= PF_GUESSED;
            }
            elem = index_in(symbols, F, sym);
            rclass = index_in(resnames, R, resn);
            if (cls == LC_HETATM) flags |= PF_HETATM;
            if (sym == 'H' || sym == 'D') flags |= PF_HYDROGEN;
            if (in_table(WATERS, resn)) flags |= PF_WATER;
            if (L[16] != ' ' && L[16] != 'A') flags |= PF_ALTLOC;
            if (std_aa) flags |= PF_STD_AA;
            if (std_aa && name == 0x20414320u) flags |= PF_CALPHA;            // " CA "
            keys[1 + r][0] = resn | (L[21] << 24);
            keys[1 + r][1] = key1;
            keys[1 + r][2] = L[26];
            if (flags & PF_BAD) atomicOr(&s_bad, 1);
        }
        __syncthreads();
        const bool has_prev = r > 0 || n_out > 0;
        const bool start = kept && (!has_prev || keys[r][0] != keys[1 + r][0] || keys[r][1] != keys[1 + r][1] || keys[r][2] != keys[1 + r][2]);
        int starts;
        const int before = block_exclusive<ST_THREADS>((int)start, part, starts);
        if (kept && fits) {
            const size_t row = (size_t)a0 + n_out + r;
            for (int c = 0; c < 3; ++c) o.pos[row * 3 + c] = pos[c];
            o.occ_b[row * 2] = ob[0];
            o.occ_b[row * 2 + 1] = ob[1];
            o.sym[row] = sym;
            o.elem[row] = elem;
            o.name[row] = name;
            o.resname[row] = resn;
            o.res_class[row] = rclass;
            o.resseq[row] = resseq;
            o.tags[row] = tags;
            o.line_off[row] = s;
            o.res_idx[row] = n_res + before + (int)start - 1;
            o.flags[row] = flags;
        }
        if (kept && r == total - 1)             // the last kept record of the chunk is the next chunk's predecessor
            for (int c = 0; c < 3; ++c) keys[0][c] = keys[total][c];
        n_out += total;
        n_res += starts;
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) {
        n_res_out[b] = n_res;
        status[b] |= (s_bad ? PS_BAD_RECORD : 0) | ((!fits && a1 > a0) ? PS_CAPACITY : 0);
    }
}

// ==== SDF / MOL V2000 text -> the layout of kpd_mol_perceive (kpd_sdf_parse) ========================================================
enum : int { SD_AROMATIC = 16, SD_CHARGES = 32, SD_V3000 = 64, SD_UNPARSABLE = 128, SD_TRUNCATED = 256, SD_LIMITS = 512 };   // beside MOL_*
constexpr int SD_RAW_MAX = 999;         // atoms a "%3d" counts line can state

// ---- per file: its records (lines between "$$$$" lines, and a last run of lines that is not all blank) -------------------------------
__global__ void __launch_bounds__(ST_THREADS)
k_sdf_count(long long n, const long long *__restrict__ fp, const int *__restrict__ n_lines_p, int cap_lines,
            const long long *__restrict__ line_start, const uint8_t *__restrict__ line_class, int *__restrict__ first_line,
            int *__restrict__ last_line, int *__restrict__ cnt, int *__restrict__ file_status) {
    __shared__ int part[ST_THREADS / 64];
    __shared__ int s_last, s_tail;
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long f0 = fp[b], f1 = fp[b + 1];
    const int nl = *n_lines_p;
    int st = 0;
    if (f0 < 0 || f1 < f0 || f1 > n) st = PS_BAD_SEGMENT;
    else if (nl > cap_lines) st = PS_LINES;
    if (st) {
        if (tid == 0) {
            first_line[b] = last_line[b] = cnt[b] = 0;
            file_status[b] = st;
        }
        return;
    }
    const int l0 = lower_bound_ll(line_start, nl, f0), l1 = lower_bound_ll(line_start, nl, f1);
    if (tid == 0) {
        s_last = l0 - 1;
        s_tail = 0;
    }
    __syncthreads();
    int seps = 0, last = l0 - 1;
    for (int k = l0 + tid; k < l1; k += ST_THREADS)
        if (line_class[k] == LC_SEP) {
            ++seps;
            last = k;
        }
    if (last >= l0) atomicMax(&s_last, last);
    __syncthreads();
    last = s_last;
    bool tail = false;
    for (int k = last + 1 + tid; k < l1 && !tail; k += ST_THREADS) tail = line_class[k] != LC_BLANK;
    if (tail) s_tail = 1;               // same-value store
    int total;
    block_exclusive<ST_THREADS>(seps, part, total);       // its barriers publish s_tail
    if (tid == 0) {
        first_line[b] = l0;
        last_line[b] = l1;
        cnt[b] = total + s_tail;
        file_status[b] = 0;
    }
}

// ---- per file: the line range and the file of every record ----------------------------------------------------------------------------
__global__ void __launch_bounds__(ST_THREADS)
k_sdf_ranges(const uint8_t *__restrict__ line_class, const int *__restrict__ first_line, const int *__restrict__ last_line,
             const int *__restrict__ mol_ptr, int cap_mols, int *__restrict__ rec_first, int *__restrict__ rec_end, int *__restrict__ rec_file,
             int *__restrict__ file_status) {
    __shared__ int part[ST_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (file_status[b] & (PS_BAD_SEGMENT | PS_LINES)) return;
    const int m0 = mol_ptr[b], m1 = mol_ptr[b + 1], l0 = first_line[b], l1 = last_line[b];
    const int cnt = m1 - m0;
    if (cnt <= 0 || m0 < 0) return;
    if (m1 > cap_mols) {
        if (tid == 0) file_status[b] |= PS_CAPACITY;
        return;                                             // nothing is written for a file whose records do not fit
    }
    if (tid == 0) {
        rec_first[m0] = l0;
        rec_end[m1 - 1] = l1;                               // the last record ends with the file unless a "$$$$" closes it (below)
    }
    for (int r = tid; r < cnt; r += ST_THREADS) rec_file[m0 + r] = b;
    __syncthreads();
    int seen = 0;
    for (int base = l0; base < l1; base += ST_THREADS) {
        const int k = base + tid;
        const bool sep = k < l1 && line_class[k] == LC_SEP;
        int total;
        const int r = seen + block_exclusive<ST_THREADS>((int)sep, part, total);
        if (sep) {
            rec_end[m0 + r] = k;                            // r < cnt: every "$$$$" closes a record
            if (r + 1 < cnt) rec_first[m0 + r + 1] = k + 1;
        }
        seen += total;
    }
}

// ---- one wave per record ---------------------------------------------------------------------------------------------------------------
struct SdfOut {
    float *pos;
    unsigned *sym;
    int *elem, *valence, *frag, *bond_ij, *bond_order;
};

__device__ __forceinline__ Line line_of(const uint8_t *__restrict__ text, const long long *__restrict__ line_start, int nl, long long fend, int k,
                                        long long &s) {
    s = line_start[k];
    long long e = k + 1 < nl ? line_start[k + 1] : fend;
    e = clamp_ll(e, s, fend > s ? fend : s);
    if (e > s && text[e - 1] == '\n') --e;
    if (e > s && text[e - 1] == '\r') --e;
    return Line{text + s, (int)(e - s < ST_COLS ? e - s : ST_COLS)};
}

__device__ __forceinline__ bool line_begins(const Line &L, const char *w, int len) {
    bool same = L.len >= len;
    for (int i = 0; i < len && same; ++i) same = L[i] == (unsigned)(unsigned char)w[i];
    return same;
}

// WRITE = false: the record's kept atoms, bonds and status (before the offsets exist).  WRITE = true: its outputs.
template <bool WRITE>
__global__ void __launch_bounds__(64)
k_sdf_records(const uint8_t *__restrict__ text, long long n, const long long *__restrict__ fp, int B, const int *__restrict__ n_lines_p,
              const long long *__restrict__ line_start, const int *__restrict__ mol_ptr, int cap_mols, const int *__restrict__ rec_first,
              const int *__restrict__ rec_end, const int *__restrict__ rec_file, const unsigned *__restrict__ symbols, int F,
              const int *__restrict__ zs, const int *__restrict__ allowed, int remove_h, int *__restrict__ cnt_atoms, int *__restrict__ cnt_bonds,
              const int *__restrict__ lig_ptr, const int *__restrict__ bond_ptr, int cap_atoms, int cap_bonds, SdfOut o,
              int *__restrict__ summary, long long *__restrict__ title_off, int *__restrict__ status) {
    __shared__ unsigned A1[MOL_MAX * MOL_W];
    __shared__ unsigned A2[MOL_MAX * MOL_W];
    __shared__ unsigned A3[MOL_MAX * MOL_W];
    __shared__ short map[SD_RAW_MAX + 1];           // raw atom -> kept atom, or -1
    __shared__ short cls[MOL_MAX];                  // class of the kept atom (F: other)
    __shared__ int label[MOL_MAX];
    __shared__ int fsize[MOL_MAX];
    const int m = blockIdx.x, lane = threadIdx.x;
    int M = mol_ptr[B];
    M = M < cap_mols ? M : cap_mols;
    const int fb = m < M ? rec_file[m] : -1;
    if (m >= M || fb < 0 || fb >= B || mol_ptr[fb + 1] > cap_mols) {        // no record here (or one of a file whose records do not fit)
        if (!WRITE && lane == 0) {
            cnt_atoms[m] = cnt_bonds[m] = 0;
            status[m] = 0;
            summary[m * 4] = summary[m * 4 + 1] = summary[m * 4 + 2] = summary[m * 4 + 3] = 0;
            title_off[m * 2] = title_off[m * 2 + 1] = 0;
        }
        return;
    }
    if (WRITE && (status[m] & MOL_BAD_SEGMENT)) return;
    const int nl = *n_lines_p, r0 = rec_first[m], r1 = rec_end[m];
    const long long fend = clamp_ll(fp[fb + 1], 0, n);
    int st = 0, na = 0, nb = 0, n_kept = 0, n_bonds = 0;
    long long s;
    bool out = r0 < 0 || r1 > nl || r1 - r0 < 4;
    if (out) st |= SD_TRUNCATED;
    if (!WRITE && lane == 0) {
        long long t0 = 0, t1 = 0;
        if (r0 >= 0 && r0 < r1 && r1 <= nl) {               // the title line's content, all of it
            t0 = line_start[r0];
            t1 = clamp_ll(r0 + 1 < nl ? line_start[r0 + 1] : fend, t0, fend > t0 ? fend : t0);
            if (t1 > t0 && text[t1 - 1] == '\n') --t1;
            if (t1 > t0 && text[t1 - 1] == '\r') --t1;
        }
        title_off[m * 2] = t0;
        title_off[m * 2 + 1] = t1;
    }
    if (!out) {
        const Line C = line_of(text, line_start, nl, fend, r0 + 3, s);
        if (line_begins(Line{C.t + 34, C.len - 34}, "V3000", 5) && C.len >= 39) {
            st |= SD_V3000;
            out = true;
        } else if (!(C.len >= 39 && line_begins(Line{C.t + 34, C.len - 34}, "V2000", 5)) || !parse_int(C, 0, 3, na) || !parse_int(C, 3, 6, nb) ||
                   na < 0 || nb < 0) {
            st |= SD_UNPARSABLE;
            out = true;
        } else if (r0 + 4 + na + nb > r1) {
            st |= SD_TRUNCATED;
            out = true;
        }
    }
    if (!out) {                                     // "M  END" behind the bond block; charge and isotope lines in front of it
        int end_at = r1;
        for (int k = r0 + 4 + na + nb + lane; k < r1 && end_at == r1; k += 64)
            if (line_begins(line_of(text, line_start, nl, fend, k, s), "M  END", 6)) end_at = k;
        end_at = wave_min_int(end_at);
        if (end_at == r1) {
            st |= SD_TRUNCATED;
            out = true;
        } else {
            bool chg = false;
            for (int k = r0 + 4 + na + nb + lane; k < end_at; k += 64) {
                const Line P = line_of(text, line_start, nl, fend, k, s);
                chg |= line_begins(P, "M  CHG", 6) || line_begins(P, "M  ISO", 6);
            }
            if (__any(chg)) st |= SD_CHARGES;
        }
    }
    const int a0 = WRITE ? lig_ptr[m] : 0, a1 = WRITE ? lig_ptr[m + 1] : 0, p0 = WRITE ? bond_ptr[m] : 0, p1 = WRITE ? bond_ptr[m + 1] : 0;
    const bool fits = WRITE && a0 >= 0 && a1 >= a0 && a1 <= cap_atoms && p0 >= 0 && p1 >= p0 && p1 <= cap_bonds;
    if (!out) {                                     // atom lines
        bool bad = false, other = false, chg = false;
        for (int base = 0; base < na; base += 64) {
            const int a = base + lane;
            bool keep = false;
            float x[3] = {0.f, 0.f, 0.f};
            unsigned sym = 0;
            int c = F;
            if (a < na) {
                const Line L = line_of(text, line_start, nl, fend, r0 + 4 + a, s);
                for (int d = 0; d < 3; ++d) bad |= !parse_real(L, 10 * d, 10 * d + 10, x[d]);
                int i = 31;
                while (i < 34 && L[i] == ' ') ++i;
                int got = 0;
                for (; i < 34 && L[i] != ' '; ++i, ++got) sym |= (got ? to_lower(L[i]) : to_upper(L[i])) << (8 * got);
                bad |= !sym;
                c = index_in(symbols, F, sym);
                int v;
                if ((parse_int(L, 34, 36, v) && v) || (parse_int(L, 36, 39, v) && v)) chg = true;
                keep = !(remove_h && (sym == 'H' || sym == 'D'));
            }
            const unsigned long long kb = __ballot(keep);
            const int idx = n_kept + __popcll(kb & ((1ull << lane) - 1ull));
            if (a < na) map[a] = (short)(keep && idx < MOL_MAX ? idx : -1);
            if (keep && idx < MOL_MAX) {
                cls[idx] = (short)c;
                if (c == F || !element_row(zs[c])) other = true;
                if (WRITE && fits && a0 + idx < a1) {
                    const size_t g = (size_t)a0 + idx;
                    for (int d = 0; d < 3; ++d) o.pos[g * 3 + d] = x[d];
                    o.sym[g] = sym;
                    o.elem[g] = c;
                }
            }
            n_kept += __popcll(kb);
        }
        if (__any(bad)) {
            st |= SD_UNPARSABLE;
            out = true;
        }
        if (__any(other)) st |= MOL_BAD_ATOM;
        if (__any(chg)) st |= SD_CHARGES;
        if (n_kept > MOL_MAX) {
            st |= SD_LIMITS;
            out = true;
        }
    }
    __syncthreads();
    if (!out) {                                     // bond lines -> the bit matrices; a bond of a dropped hydrogen goes with it
        for (int k = lane; k < n_kept * MOL_W; k += 64) A1[k] = A2[k] = A3[k] = 0;
        __syncthreads();
        bool bad = false, dup = false, arom = false;
        for (int q = lane; q < nb; q += 64) {
            const Line L = line_of(text, line_start, nl, fend, r0 + 4 + na + q, s);
            int i, j, t;
            if (!parse_int(L, 0, 3, i) || !parse_int(L, 3, 6, j) || !parse_int(L, 6, 9, t) || i < 1 || j < 1 || i > na || j > na || t < 1 || t > 4) {
                bad = true;                         // also the query types 5 .. 8
                continue;
            }
            if (i == j) {
                dup = true;
                continue;
            }
            if (t == 4) {
                arom = true;
                t = 1;
            }
            int u = map[i - 1], v = map[j - 1];
            if (u < 0 || v < 0) continue;
            if (u > v) {
                const int w = u;
                u = v;
                v = w;
            }
            const unsigned old = atomicOr(&A1[u * MOL_W + (v >> 5)], 1u << (v & 31));
            if (old & (1u << (v & 31))) {
                dup = true;
                continue;
            }
            atomicOr(&A1[v * MOL_W + (u >> 5)], 1u << (u & 31));
            if (t >= 2) {
                atomicOr(&A2[u * MOL_W + (v >> 5)], 1u << (v & 31));
                atomicOr(&A2[v * MOL_W + (u >> 5)], 1u << (u & 31));
            }
            if (t >= 3) {
                atomicOr(&A3[u * MOL_W + (v >> 5)], 1u << (v & 31));
                atomicOr(&A3[v * MOL_W + (u >> 5)], 1u << (u & 31));
            }
        }
        __syncthreads();
        int deg_sum = 0;
        bool wide = false;
        for (int i = lane; i < n_kept; i += 64) {
            int d = 0;
            for (int w = 0; w < MOL_W; ++w) d += __popc(A1[i * MOL_W + w]);
            wide |= d > MOL_DEG;
            deg_sum += d;
        }
        n_bonds = wave_sum(deg_sum) / 2;
        if (__any(bad)) st |= SD_UNPARSABLE;
        if (__any(dup) || __any(wide) || n_bonds > 3 * n_kept) st |= SD_LIMITS;
        if (__any(arom)) st |= SD_AROMATIC;
        out = (st & (SD_UNPARSABLE | SD_LIMITS)) != 0;
    }
    if (out) {
        st = (st & ~(MOL_BAD_ATOM | SD_AROMATIC)) | MOL_BAD_SEGMENT;
        n_kept = n_bonds = 0;
    } else if (n_kept == 0) {
        st |= MOL_EMPTY;
    }
    if (!WRITE) {
        if (lane == 0) {
            cnt_atoms[m] = n_kept;
            cnt_bonds[m] = n_bonds;
            status[m] = st;
            summary[m * 4] = summary[m * 4 + 1] = summary[m * 4 + 2] = summary[m * 4 + 3] = 0;
        }
        return;
    }
    if (out || n_kept == 0) return;
    if (!fits || a1 - a0 != n_kept || p1 - p0 != n_bonds) {
        if (lane == 0) status[m] = st | MOL_CAPACITY;       // nothing more is written for a record that does not fit
        return;
    }
    int n_frags, largest, invalid, total;
    mol_fragments_out(A1, A2, A3, label, fsize, n_kept, lane, a0,
                      [&](int k, int val) {
                          const int c = cls[lane + 64 * k];
                          return val == 0 || c == F || !element_row(zs[c]) || val > allowed[c];
                      },
                      o.valence, o.frag, o.bond_ij + (size_t)2 * p0, o.bond_order + p0, n_frags, largest, invalid, total);
    if (lane == 0) {
        summary[m * 4] = total;
        summary[m * 4 + 1] = n_frags;
        summary[m * 4 + 2] = largest;
        summary[m * 4 + 3] = invalid;
    }
}

}  // namespace kpd

using namespace kpd;

// line counts and offsets of the tiles, the line table, and per file: first line, line of the first ENDMDL, kept records
struct PdbScratch {
    long long n_bytes;
    int B, cap_lines;
    int *tile_cnt = nullptr, *tile_ptr = nullptr, *first_line = nullptr, *end_line = nullptr, *cnt = nullptr;
    long long *line_start = nullptr;
    uint8_t *line_class = nullptr;
    size_t tiles() const { return (size_t)((n_bytes + 15 + ST_TILE - 1) / ST_TILE); }
    void operator()(Carve &c) {
        c(tile_cnt, tiles()); c(tile_ptr, tiles() + 1); c(line_start, cap_lines); c(line_class, cap_lines);
        c(first_line, B); c(end_line, B); c(cnt, B);
    }
};

static bool pdb_sizes_ok(int64_t n_bytes, int32_t B, int32_t cap_lines) {
    return n_bytes >= 0 && B >= 0 && cap_lines >= 0 && n_bytes + B < 0x7fffffffLL;
}

extern "C" int64_t kpd_pdb_scratch_bytes(int64_t n_bytes, int32_t B, int32_t cap_lines) {
    if (!pdb_sizes_ok(n_bytes, B, cap_lines)) return -1;
    PdbScratch s{n_bytes, B, cap_lines};
    return scratch_bytes(s);
}

extern "C" kpd_status kpd_pdb_parse(const uint8_t *text, int64_t n_bytes, const int64_t *file_ptr, int32_t B, const uint32_t *symbols,
                                    int32_t F, const uint32_t *resnames, int32_t R, int32_t cap_lines, int32_t cap_atoms, float *pos,
                                    float *occ_b, uint32_t *sym, int32_t *elem, uint32_t *name, uint32_t *resname, int32_t *res_class,
                                    int32_t *resseq, uint32_t *tags, int64_t *line_off, int32_t *res_idx, int32_t *flags,
                                    int32_t *atom_ptr, int32_t *n_res, int32_t *status, int32_t *n_lines, void *scratch, void *stream) {
    KPD_REQUIRE(n_bytes >= 0 && B >= 0 && F >= 0 && R >= 0 && cap_lines >= 0 && cap_atoms >= 0, KPD_ERR_INVALID,
                "n_bytes=%lld B=%d F=%d R=%d cap_lines=%d cap_atoms=%d", (long long)n_bytes, B, F, R, cap_lines, cap_atoms);
    KPD_REQUIRE(pdb_sizes_ok(n_bytes, B, cap_lines), KPD_ERR_CAPACITY, "n_bytes + B = %lld: at most 2^31 - 2 per call", (long long)n_bytes + B);
    KPD_REQUIRE(file_ptr && atom_ptr && n_lines && scratch && (!B || (n_res && status)), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE((!n_bytes || text) && (!F || symbols) && (!R || resnames), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!cap_atoms || (pos && occ_b && sym && elem && name && resname && res_class && resseq && tags && line_off && res_idx && flags),
                KPD_ERR_INVALID, "null output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PdbScratch s{n_bytes, B, cap_lines};
    carve_raw(static_cast<char *>(scratch), s);
    const long long *fp = reinterpret_cast<const long long *>(file_ptr);
    const int tiles = n_bytes ? (int)((n_bytes + (long long)(reinterpret_cast<uintptr_t>(text) & 15) + ST_TILE - 1) / ST_TILE) : 0;
    if (tiles) {
        hipLaunchKernelGGL(k_struct_count, dim3(tiles), dim3(ST_THREADS), 0, st, text, (long long)n_bytes, fp, B, s.tile_cnt);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, s.tile_cnt, tiles, s.tile_ptr, (int *)nullptr, StoreTotal{n_lines}));
    if (tiles) {
        hipLaunchKernelGGL(k_struct_lines, dim3(tiles), dim3(ST_THREADS), 0, st, text, (long long)n_bytes, fp, B, s.tile_ptr, cap_lines, 0,
                           s.line_start, s.line_class);
        KPD_LAUNCH_CHECK();
    }
    if (B) {
        hipLaunchKernelGGL(k_pdb_count, dim3(B), dim3(ST_THREADS), 0, st, (long long)n_bytes, fp, n_lines, cap_lines, s.line_start, s.line_class,
                           s.first_line, s.end_line, s.cnt, status);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, s.cnt, B, atom_ptr));
    if (B) {
        PdbOut o{pos, occ_b, sym, elem, name, resname, res_class, resseq, tags, reinterpret_cast<long long *>(line_off), res_idx, flags};
        hipLaunchKernelGGL(k_pdb_records, dim3(B), dim3(ST_THREADS), 0, st, text, (long long)n_bytes, fp, n_lines, s.line_start, s.line_class,
                           s.first_line, s.end_line, symbols, F, resnames, R, atom_ptr, cap_atoms, o, n_res, status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}

// the line table as for kpd_pdb_parse; per file: lines and records; per record: lines, file, kept atoms and bonds
struct SdfParseScratch {
    long long n_bytes;
    int B, cap_lines, cap_mols;
    int *tile_cnt = nullptr, *tile_ptr = nullptr, *first_line = nullptr, *last_line = nullptr, *cnt = nullptr;
    int *rec_first = nullptr, *rec_end = nullptr, *rec_file = nullptr, *cnt_atoms = nullptr, *cnt_bonds = nullptr;
    long long *line_start = nullptr;
    uint8_t *line_class = nullptr;
    size_t tiles() const { return (size_t)((n_bytes + 15 + ST_TILE - 1) / ST_TILE); }
    void operator()(Carve &c) {
        c(tile_cnt, tiles()); c(tile_ptr, tiles() + 1); c(line_start, cap_lines); c(line_class, cap_lines);
        c(first_line, B); c(last_line, B); c(cnt, B);
        c(rec_first, cap_mols); c(rec_end, cap_mols); c(rec_file, cap_mols); c(cnt_atoms, cap_mols); c(cnt_bonds, cap_mols);
    }
};

extern "C" int64_t kpd_sdf_parse_scratch_bytes(int64_t n_bytes, int32_t B, int32_t cap_lines, int32_t cap_mols) {
    if (!pdb_sizes_ok(n_bytes, B, cap_lines) || cap_mols < 0) return -1;
    SdfParseScratch s{n_bytes, B, cap_lines, cap_mols};
    return scratch_bytes(s);
}

extern "C" kpd_status kpd_sdf_parse(const uint8_t *text, int64_t n_bytes, const int64_t *file_ptr, int32_t B, const uint32_t *symbols,
                                    int32_t F, const int32_t *z, const int32_t *allowed, int32_t remove_h, int32_t cap_lines,
                                    int32_t cap_mols, int32_t cap_atoms, int32_t cap_bonds, int32_t *mol_ptr, int32_t *file_status,
                                    int32_t *lig_ptr, float *pos, uint32_t *sym, int32_t *elem, int32_t *valence, int32_t *frag,
                                    int32_t *bond_ij, int32_t *bond_order, int32_t *bond_ptr, int32_t *summary, int64_t *title_off,
                                    int32_t *status, int32_t *n_lines, void *scratch, void *stream) {
    KPD_REQUIRE(n_bytes >= 0 && B >= 0 && F >= 1 && cap_lines >= 0 && cap_mols >= 0 && cap_atoms >= 0 && cap_bonds >= 0, KPD_ERR_INVALID,
                "n_bytes=%lld B=%d F=%d cap_lines=%d cap_mols=%d cap_atoms=%d cap_bonds=%d", (long long)n_bytes, B, F, cap_lines, cap_mols,
                cap_atoms, cap_bonds);
    KPD_REQUIRE(pdb_sizes_ok(n_bytes, B, cap_lines), KPD_ERR_CAPACITY, "n_bytes + B = %lld: at most 2^31 - 2 per call", (long long)n_bytes + B);
    KPD_REQUIRE(file_ptr && mol_ptr && lig_ptr && bond_ptr && n_lines && scratch && symbols && z && allowed && (!B || file_status),
                KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE((!n_bytes || text) && (!cap_mols || (summary && title_off && status)), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE((!cap_atoms || (pos && sym && elem && valence && frag)) && (!cap_bonds || (bond_ij && bond_order)), KPD_ERR_INVALID, "null output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    SdfParseScratch s{n_bytes, B, cap_lines, cap_mols};
    carve_raw(static_cast<char *>(scratch), s);
    const long long *fp = reinterpret_cast<const long long *>(file_ptr);
    const int tiles = n_bytes ? (int)((n_bytes + (long long)(reinterpret_cast<uintptr_t>(text) & 15) + ST_TILE - 1) / ST_TILE) : 0;
    if (tiles) {
        hipLaunchKernelGGL(k_struct_count, dim3(tiles), dim3(ST_THREADS), 0, st, text, (long long)n_bytes, fp, B, s.tile_cnt);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, s.tile_cnt, tiles, s.tile_ptr, (int *)nullptr, StoreTotal{n_lines}));
    if (tiles) {
        hipLaunchKernelGGL(k_struct_lines, dim3(tiles), dim3(ST_THREADS), 0, st, text, (long long)n_bytes, fp, B, s.tile_ptr, cap_lines, 1,
                           s.line_start, s.line_class);
        KPD_LAUNCH_CHECK();
    }
    if (B) {
        hipLaunchKernelGGL(k_sdf_count, dim3(B), dim3(ST_THREADS), 0, st, (long long)n_bytes, fp, n_lines, cap_lines, s.line_start, s.line_class,
                           s.first_line, s.last_line, s.cnt, file_status);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, s.cnt, B, mol_ptr));
    if (cap_mols) KPD_HIP(hipMemsetAsync(s.rec_file, 0xff, (size_t)cap_mols * 4, st));        // -1: no record
    if (B) {
        hipLaunchKernelGGL(k_sdf_ranges, dim3(B), dim3(ST_THREADS), 0, st, s.line_class, s.first_line, s.last_line, mol_ptr, cap_mols,
                           s.rec_first, s.rec_end, s.rec_file, file_status);
        KPD_LAUNCH_CHECK();
    }
    SdfOut o{pos, sym, elem, valence, frag, bond_ij, bond_order};
    long long *toff = reinterpret_cast<long long *>(title_off);
    if (cap_mols) {
        hipLaunchKernelGGL(k_sdf_records<false>, dim3(cap_mols), dim3(64), 0, st, text, (long long)n_bytes, fp, B, n_lines, s.line_start, mol_ptr,
                           cap_mols, s.rec_first, s.rec_end, s.rec_file, symbols, F, z, allowed, remove_h, s.cnt_atoms, s.cnt_bonds, lig_ptr,
                           bond_ptr, cap_atoms, cap_bonds, o, summary, toff, status);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, s.cnt_atoms, cap_mols, lig_ptr));
    KPD_TRY(exclusive_scan(st, s.cnt_bonds, cap_mols, bond_ptr));
    if (cap_mols) {
        hipLaunchKernelGGL(k_sdf_records<true>, dim3(cap_mols), dim3(64), 0, st, text, (long long)n_bytes, fp, B, n_lines, s.line_start, mol_ptr,
                           cap_mols, s.rec_first, s.rec_end, s.rec_file, symbols, F, z, allowed, remove_h, s.cnt_atoms, s.cnt_bonds, lig_ptr,
                           bond_ptr, cap_atoms, cap_bonds, o, summary, toff, status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}
