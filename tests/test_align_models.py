"""CPU checks of the alignment kernel's arithmetic (no GPU): the closed form of Zoe's lazy-F loop (striped.rs:528-553)
and the packed row update the gfx950 kernel is compiled from (zoe_amd/csrc/zsw_align_pk.hpp), both compared cell by
cell with the oracle's literal restatement of sw_simd_align; the bound checks of the column-pruned first pass
(zoe_amd/csrc/zsw_score_prune.hip) against the full DP matrix; and the alignment certificates (zoe_amd/csrc/zsw_cert.hpp) against
counting Gotoh and the literal sw_simd_align, with mutants of the header that the models must catch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_built = {}


def _build(tmp_path, name):
    """Compiles tests/models/<name>.cpp once per session (the twin instantiates 6 lane counts x 12 vector counts)."""
    if name not in _built:
        import tempfile

        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_models_"), name)
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "models", name + ".cpp")], check=True)
        _built[name] = exe
    return _built[name]


@pytest.mark.parametrize("seed", [20261004, 7])
def test_closed_form_lazy_f_equals_the_literal_loop(tmp_path, seed):
    """T = (round, vector) of the loop's break from per-round bit strings, flags and H from M(v, lane): identical striped
    backtrack matrices for N = 2..64, ten scoring schemes (gap_open = 0, gap_extend = 0 and equal gaps among them)."""
    out = subprocess.run([_build(tmp_path, "align_closed_form"), "120", str(seed)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.parametrize("seed", [20261004, 99])
def test_packed_row_update_twin_equals_the_oracle(tmp_path, seed):
    """zsw_align_pk.hpp compiled for the host (64 explicit lanes, the plain-C meaning of each gfx950 instruction): 2*64/N reads
    per wavefront with different lengths and last rows, the first rows through the flag-less scan path."""
    out = subprocess.run([_build(tmp_path, "align_pk_twin"), "5", str(seed)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.parametrize("seed", [20261004, 5, 77])
def test_pruning_bounds_model(tmp_path, seed):
    """The claim the column-pruned first pass rests on (zoe_amd/csrc/zsw_score_prune.hip), with plain integers against the full
    Gotoh matrix: a read that passes the three bound checks has the true maximum (and, with the strict checks, the true first
    row and column); strips of 8-48 columns, six scoring schemes (free gaps and gap_extend 0 among them), repeats, second
    copies, long gaps, junk ends, reads hanging over the reference ends."""
    out = subprocess.run([_build(tmp_path, "prune_bounds"), "80", str(seed)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "prune_bounds OK" in out.stdout


@pytest.mark.parametrize("seed", [20261004, 11, 314])
def test_seeded_pass_bounds_model(tmp_path, seed):
    """The claims the seeded exact pass rests on (zoe_amd/csrc/zsw_seed.hpp, compiled for the host as the kernels compile it),
    with plain integers against the full Gotoh matrix: no path that starts above the window, starts below it, or leaves it through
    the last row beats its bound — checked for every read against DPs restricted to each class of paths — and a read that passes
    has the true maximum (with the strict checks: the true first row and column). Eight scoring schemes (free extension, N scored
    -1 / +1), k = 3..6 on references of 60-420 bases so that chance k-mer hits abound, repeats, tandem repeats, N runs, chimeras,
    long gaps, reads hanging over the ends."""
    out = subprocess.run([_build(tmp_path, "seed_bounds"), "400", str(seed)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "seed_bounds OK" in out.stdout


@pytest.mark.parametrize("seed", [20261004, 23])
def test_late_start_certificate_model(tmp_path, seed):
    """The certificate that lets the alignment's second pass start a few rows above the alignment instead of warmup_rows above
    it (zsw_seed.hpp: seed_safe_start): Zoe's own striped alignment (the oracle's sw_simd_align at <i16, 4 / 8 / 16>) of a read
    against reference[r0..] equals its alignment against the whole reference, shifted by r0 — score, ranges and CIGAR — for every
    read that gets a certificate; seven scoring schemes, repeats, tandem repeats, N, junk prefixes, long deletions."""
    out = subprocess.run([_build(tmp_path, "seed_warmup"), "400", str(seed)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "seed_warmup OK" in out.stdout


@pytest.mark.parametrize("seed", [20261004, 7, 41])
def test_banded_pass_bounds_model(tmp_path, seed):
    """The banded form of the seeded pass (zoe_amd/csrc/zsw_score_band.hip) in its injected form (zsw_seed.hpp, "banded pass"):
    what enters the band from outside is an upper bound of the outside cell's value — from two bound programmes along the query
    columns, one per side (seed_col_step / seed_col_join / seed_strip_events / seed_exit_is_free) —, doubled and made odd, so that
    an even maximum is the score of a real path inside the band that no path through an outside cell reaches. The model walks
    a read as the kernel does and checks against the full Gotoh matrix, for every read whether accepted or not: every cell of the
    band holds a bound >= its true H; every cell above / below the band is <= a(c) / b(c) of its column and <= oa / ob; what the
    next strip's first column receives covers the cells left of it; per class of paths (wholly outside; leaving strip k through
    its right edge / its last row) the class's best path stays under the bound programme of that class alone, so that a weak
    bound cannot hide behind a larger one; an accepted read has the true score (ends tag: the true first row and column, and the
    true number of cells holding the maximum). Copies with 0-12 % substitutions + indels, chimeras, long deletions / insertions,
    overhanging and random reads, structured cases (residues without potential between the sampled k-mers, tests/models/
    adversarial_reads.hpp); eleven schemes (free gap extension, mismatch loss >= gap_open); strips of 5-32 columns, bands of a few
    diagonals, lane partners that widen the band or add strips of padding."""
    out = subprocess.run([_build(tmp_path, "seed_band"), "250", str(seed)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "seed_band OK" in out.stdout


@pytest.mark.parametrize("seed", [3, 20261005])
def test_reversed_pass_over_whole_sequences_model(tmp_path, seed):
    """The shared role's sw_score_ranges runs its second pass over the whole reversed sequences (a seeded pass) instead of the
    reversed prefixes of striped.rs:355-388 and accepts a read only if the forward maximum and the reversed maximum each sit in
    one cell (zsw_capi_shared.hip, settle_reverse_kernel). Claim, against plain Gotoh matrices: with the forward maximum in one
    cell, the cells holding the score in the reversed matrix of the prefixes and of the whole sequences are the same positions —
    random schemes (asymmetric matrices, N scoring -1/0/+1, free gap extension), repeats, low-complexity pairs."""
    out = subprocess.run([_build(tmp_path, "reverse_unique"), "4000", str(seed)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reverse_unique OK" in out.stdout


@pytest.mark.parametrize("seed", [20261005, 8])
def test_gapless_alignment_certificate_model(tmp_path, seed):
    """The gapless certificate that lets sw_simd_align's second pass be skipped (zoe_amd/csrc/zsw_cert.hpp, compiled for the host as
    the classify pass of zsw_threepass.hip compiles it, with its split into a classify and a sweep launch): both maxima in one cell
    each, ranges of equal length n whose diagonal adds up to the score S, S > maxw * (n - 1) - 3 * gap_open (three or more gap runs),
    and for every run length k with maxw * (n - k) - 2 * gap_open - 2 * (k - 1) * gap_extend >= S the best placement of an insertion and
    a deletion of k below S (one sweep per k and order). Every certificate is checked against a Gotoh that counts the optimal
    alignments between the corners (exactly one) and against the oracle's literal sw_simd_align at N = 2 .. 64 in i16 lanes, N = 16,
    32 in i8 and u8 lanes, N = 4, 16 in u16 lanes, N = 8 in i32 and u32 lanes, and with the roles swapped; sixteen schemes (an
    asymmetric matrix, three letters, gap_extend 0 and == gap_open among them), repeats, homopolymer runs, N, junk ends, indel pairs
    of the same length a few bases apart, substitution counts around the potential's threshold."""
    out = subprocess.run([_build(tmp_path, "align_gapless_cert"), "250", str(seed)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "align_gapless_cert OK" in out.stdout


@pytest.mark.parametrize("seed", [20261005, 6])
def test_one_gap_alignment_certificate_model(tmp_path, seed):
    """The one-gap certificate (zsw_cert.hpp as above): both maxima in one cell each, ranges that differ by g, m = min(rlen, qlen) >= 2,
    gap_extend > 0, S > maxw * m - 3 * gap_open - max(g - 3, 0) * gap_extend (three or more runs), one placement of ONE gap run of g
    between the corners — or a run of adjacent placements, of which the walk from the end takes the last — reaches exactly S (one sweep
    over the prefix sums of the two diagonals), and for every pair of runs (ra, rlen - qlen - ra) with |ra| <= amax that the potential
    does not rule out the best placement stays below S. Every certificate is checked against a Gotoh that counts the optimal alignments
    between the corners (exactly the tied placements) and against the oracle's literal sw_simd_align at the widths above and with the
    roles swapped; sixteen schemes, gaps of 1-5 inside repeats and homopolymer runs (tied placements), second indels a few bases away
    (two runs at exactly S) and farther away (around amax)."""
    out = subprocess.run([_build(tmp_path, "align_onegap_cert"), "250", str(seed)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "align_onegap_cert OK" in out.stdout


# One textual change each to zsw_cert.hpp (the target text occurs exactly once), the model that must then fail, and its seed.
# (amax one smaller is provably harmless: a pair of runs within reach of S has |ra| <= (X + g) / 2, and amax carries a margin of one.)
CERT_MUTANTS = [
    ("the gapless sweep's verdict ignored", "                if (cert_gapless_two_runs(wt, rlen, k, dir, c)) {",
     "                if (false && cert_gapless_two_runs(wt, rlen, k, dir, c)) {", "align_gapless_cert", 20261005),
    ("deferred one-gap reads certified without the sweep launch",
     "            r.verdict = CERT_DEFERRED;\n            r.deferred = true;\n            return r;\n        }\n        if (cert_one",
     "            r.verdict = CERT_ONE_GAP;\n            return r;\n        }\n        if (cert_one", "align_onegap_cert", 20261005),
    ("the first tied placement instead of the last", "    r.param = (int32_t)best_p;", "    r.param = (int32_t)first_p;",
     "align_onegap_cert", 20261005),
    (">= S becomes > S in the one-gap two-run rejection", "    return pzM - cost + best_alt >= S;", "    return pzM - cost + best_alt > S;",
     "align_onegap_cert", 20261005),
    (">= S becomes > S in the gapless two-run rejection", "c.ge * ((long long)k - 1) >= 0;", "c.ge * ((long long)k - 1) > 0;",
     "align_gapless_cert", 20261005),
    ("amax two smaller", "(X + g) / 2 + 1 : 0", "(X + g) / 2 - 1 : 0", "align_onegap_cert", 20261005),
    ("3 * gap_open becomes 2 * gap_open in the gapless three-run potential",
     "    return (long long)score > c.maxw * ((long long)n - 1) - 3ll * c.go;",
     "    return (long long)score > c.maxw * ((long long)n - 1) - 2ll * c.go;", "align_gapless_cert", 20261005),
]


@pytest.mark.parametrize("name,old,new,model,seed", CERT_MUTANTS, ids=[m[0] for m in CERT_MUTANTS])
def test_certificate_models_kill_mutants_of_the_shipped_header(tmp_path, name, old, new, model, seed):
    """The models have teeth: each mutant of zsw_cert.hpp, compiled into the model with a reduced set of widths (<i16, 16> and the
    swapped <i16, 8>), makes the model fail at the committed iteration count — a certificate whose optimal alignments between the corners
    are not the certified ones, one that the literal sw_simd_align does not return, or (3 * gap_open -> 2 * gap_open, which only loses
    certificates) no read left that needs the sweeps."""
    src = open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_cert.hpp")).read()
    assert src.count(old) == 1, f"mutation target of {name!r} is not unique in zsw_cert.hpp"
    header = tmp_path / "zsw_cert.hpp"
    header.write_text(src.replace(old, new))
    exe = str(tmp_path / model)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-DZSW_CERT_FEW_WIDTHS", f'-DZSW_CERT_HEADER="{header}"', "-o", exe,
                    os.path.join(ROOT, "tests", "models", model + ".cpp")], check=True)
    out = subprocess.run([exe, "250", str(seed)], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode != 0, f"mutant survived: {name}\n{out.stdout}"
    assert f"{model} OK" not in out.stdout


@pytest.mark.parametrize("seed", [20261005, 4])
def test_row_chunked_full_pass_model(tmp_path, seed):
    """Reads the seeded pass hands back against a long reference are scored in chunks of rows, each from a zero state with an
    overlap of L + L * maxw / gap_extend + 2 rows (zsw_score_v2.hpp, ScoreArgsV2::chunk_rows): the largest (score, earliest row,
    earliest column) over the chunks is the whole matrix's, with repeats in the reference and long deletions in the reads."""
    out = subprocess.run([_build(tmp_path, "chunk_rows"), "2500", str(seed)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "chunk_rows OK" in out.stdout
