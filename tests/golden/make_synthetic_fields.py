"""Generate tests/golden/synthetic_fields.json: moduli that reach the kernel branches the
reference's own fields (fields.json) never do.

rg_field_create takes any odd modulus of 1, 2, 4, 7 or 14 limbs, but every field of the reference
has q mod 2^32 == 1, a spare top bit (bar mult_zp) and, at one limb, 62.1 bits.  The primes here
are each the LARGEST one satisfying a stated rule, found by downward search with pyref.is_prime
only, so anyone can reproduce them; two are fixed well-known values.  Every one has
2-adicity >= 17, so the negacyclic transform of rank 2^16 exists for all of them.

The output is DATA (q, bits, limbs, 2-adicity of q - 1, q mod 2^32, the rule); the oracle and
the library derive every constant themselves.  fields.json stays the record of the reference's
fields; this file is separate on purpose.  Running the script rewrites the JSON byte for byte.
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "oracle"))
import pyref  # noqa: E402


def largest_prime(bound, step, lo32_is_one):
    """Largest prime q < bound with q = 1 mod step and (q mod 2^32 == 1) == lo32_is_one."""
    q = (bound - 2) // step * step + 1
    while q > 1:
        if ((q & 0xFFFFFFFF) == 1) == lo32_is_one and pyref.is_prime(q):
            return q
        q -= step
    raise ValueError("no prime")


# name -> (prime, rule, the branch it reaches)
def specs():
    return [
        ("s30", 7 * 2 ** 26 + 1, "fixed: 7 * 2^26 + 1",
         "L=1 Shoup, QLO1=false, small q"),
        ("s62_lo", largest_prime(2 ** 62, 2 ** 17, False), "largest q < 2^62, q = 1 mod 2^17, q mod 2^32 != 1",
         "L=1 Shoup, QLO1=false, generic two-pass plan at 2^16"),
        ("s63_top", largest_prime(2 ** 63, 2 ** 32, True), "largest q < 2^63, q = 1 mod 2^32",
         "lazy ntt16_pass with 3q > 2^64"),
        ("s64_gold", 2 ** 64 - 2 ** 32 + 1, "fixed: 2^64 - 2^32 + 1 (Goldilocks)",
         "L=1 non-Shoup (Montgomery), q mod 2^32 == 1"),
        ("s64_lo", largest_prime(2 ** 64, 2 ** 17, False), "largest q < 2^64, q = 1 mod 2^17, q mod 2^32 != 1",
         "L=1 non-Shoup (Montgomery), q mod 2^32 != 1"),
        ("s256_top", largest_prime(2 ** 256, 2 ** 64, True), "largest q < 2^256, q = 1 mod 2^64",
         "L=4, q[0] == 1 but top bit set: the ntt256 fast path must decline"),
        ("s256_lo", largest_prime(2 ** 256, 2 ** 17, False), "largest q < 2^256, q = 1 mod 2^17, q mod 2^32 != 1",
         "L=4 generic plan, no spare bit, q[0] != 1"),
        ("s448_top", largest_prime(2 ** 448, 2 ** 64, True), "largest q < 2^448, q = 1 mod 2^64",
         "L=7 without a spare bit: per-stage kernels"),
        ("s896_top", largest_prime(2 ** 896, 2 ** 64, True), "largest q < 2^896, q = 1 mod 2^64",
         "L=14 without a spare bit: per-stage kernels"),
    ]


def two_adicity(q):
    n, k = q - 1, 0
    while n % 2 == 0:
        n //= 2
        k += 1
    return k


def main(out):
    fields = {}
    for name, q, rule, branch in specs():
        assert pyref.is_prime(q), name
        fields[name] = {"q_hex": hex(q), "bits": q.bit_length(), "limbs": (q.bit_length() + 63) // 64,
                        "two_adicity": two_adicity(q), "q_mod_2_32": q & 0xFFFFFFFF, "rule": rule, "branch": branch}
    with open(out, "w") as f:
        json.dump(fields, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, sorted(fields))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                              "synthetic_fields.json"))
