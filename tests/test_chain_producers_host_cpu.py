"""No GPU: the host's choice between the two forms in which the producers of the lean halo chain kernel take the logits
(h1_lean_input, end2end_amd/csrc/ctc_loss_fast_h1.hip, through e2e_debug_chain_lean_input).  The lean form adds 32-bit byte
offsets to an utterance's base address and multiplies a row number by four times the row stride in 24 bits, so it is only for
shapes on which that arithmetic cannot wrap; a view whose T * sT passes 2^31 elements cannot be allocated in a test, so the
rule is checked here, against its statement, on both sides of each bound."""

from end2end_amd import _lib


def lean(dtype, T, V, sT, sV=1):
    L = _lib.load()
    return L.e2e_debug_chain_lean_input(dtype, T, V, sT, sV)


def stated(dtype, T, V, sT, sV):
    """the rule as include/e2e_ctc_debug.h states it"""
    return int(dtype == _lib.F32 and sV == 1 and 0 <= sT < 2 ** 22 and 1 <= T < 2 ** 24
               and ((T - 1) * sT + V + 8) * 4 < 2 ** 31 and -(-T // 16) * 16 * V * 4 < 2 ** 31)


def test_the_headline_shape_and_the_tests_shapes_are_lean():
    assert lean(_lib.F32, 1000, 29, 29) == 1
    for T in (1, 2, 7, 8, 9, 73, 200):
        for V in (2, 29, 78):
            assert lean(_lib.F32, T, V, V) == 1
            assert lean(_lib.F32, T, V, 40 if V <= 40 else V + 7) == 1          # rows padded


def test_other_dtypes_and_strided_columns_keep_64_bit_offsets():
    for dt in (_lib.F16, _lib.BF16, _lib.F64):
        assert lean(dt, 1000, 29, 29) == 0
    assert lean(_lib.F32, 1000, 29, 58, 2) == 0
    assert lean(_lib.F32, 1000, 29, 29, 0) == 0
    assert lean(_lib.F32, 1000, 29, -29) == 0              # rows stored backwards
    assert lean(_lib.F32, 1000, 29, 0) == 1                # every frame the same row: offsets stay inside one row


def test_the_bounds_of_the_32_bit_arithmetic():
    V = 29
    # the logits' byte offsets: ((T - 1) sT + V + 8) * 4 < 2^31
    for T, sT in ((1000, (2 ** 29 - V - 8) // 999), (2 ** 20, 511), (2 ** 20, 512), (3, 2 ** 22 - 1), (3, 2 ** 22)):
        for d in (-1, 0, 1):
            assert lean(_lib.F32, T, V, sT + d) == stated(_lib.F32, T, V, sT + d, 1), (T, sT + d)
    t_edge = (2 ** 29 - V - 8) // 64 + 1                  # rows 64 apart: the first T whose last row passes the bound
    assert [lean(_lib.F32, t_edge + d, V, 64) for d in (-1, 0, 1, 2)] == [stated(_lib.F32, t_edge + d, V, 64, 1) for d in (-1, 0, 1, 2)]
    assert lean(_lib.F32, t_edge - 1, V, 64) == 1 and lean(_lib.F32, t_edge + 2, V, 64) == 0
    # the row stride times four as a 24-bit factor
    assert lean(_lib.F32, 2, V, 2 ** 22 - 1) == 1 and lean(_lib.F32, 2, V, 2 ** 22) == 0
    # a view of T * sT > 2^31 elements, as the issue's list has it
    assert lean(_lib.F32, 1000, V, 2 ** 22 - 1) == 0 and lean(_lib.F32, 2 ** 12, V, 2 ** 20) == 0
    # the probability table's bytes per utterance (rows overlapping, sT = 1, so that only this bound is in play)
    t_y = 2 ** 31 // (78 * 4) // 16 * 16
    for T in (t_y - 16, t_y, t_y + 1, t_y + 16):
        assert lean(_lib.F32, T, 78, 1) == stated(_lib.F32, T, 78, 1, 1), T
    assert lean(_lib.F32, t_y, 78, 1) == 1 and lean(_lib.F32, t_y + 16, 78, 1) == 0
    assert lean(_lib.F32, 0, V, 29) == 0 and lean(_lib.F32, 2 ** 24, 2, 0) == 0


def test_the_rule_on_a_grid():
    for dt in (_lib.F32, _lib.F16):
        for T in (1, 999, 2 ** 16, 2 ** 24 - 1):
            for V in (2, 29, 78):
                for sT in (0, V, 4096, 2 ** 16, 2 ** 22 - 1, 2 ** 30):
                    for sV in (1, 2):
                        assert lean(dt, T, V, sT, sV) == stated(dt, T, V, sT, sV), (dt, T, V, sT, sV)
