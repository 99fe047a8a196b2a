"""fmt_float of fastplong_amd/csrc/bam_comment_rules.h -- the "%g" of a float in integer arithmetic, for host and device -- against
the libc, in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (tests/host_bamcomment): every exponent
with both signs under fixed and 4096 seeded random mantissas, every exact tie at six digits."""
from tests.host_bamcomment import build as floatcheck


def test_fmt_float_is_the_libc_s_g_on_every_input():
    checked, bad, longest, report = floatcheck.check(seed=20240607)
    # 2 x 256 x (4 + 4096) + 2 x 900 000 ties n + 0.5 + 2 x 900 000 values 10 k + 5
    assert checked == 2 * 256 * 4100 + 2 * 900000 + 2 * 900000
    assert bad == 0, report
    assert longest == 12
