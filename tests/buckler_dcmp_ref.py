"""Test reference for the Buckler norm decomposition: a Python restatement of buckler/utils.go:34-56
and buckler/prover.go:77-111, 182-192, loop by loop and in the reference's order, over Python
integers.  It works over buckler_lin_ref.Ref (Montgomery-form ints) and reuses its decomposeBase.

A witness is a list of Montgomery-form ints, as everywhere in buckler_lin_ref."""
from tests.buckler_lin_ref import decomposeBase  # noqa: F401  (utils.go:7-32)


# ---- utils.go:34-56 ----------------------------------------------------------------------------------
def decomposeBig(x, base, q):
    xSigned = x
    qHalf = q >> 1
    if xSigned > qHalf:
        xSigned = xSigned - q
    dcmpOut = [0] * len(base)
    for i in range(len(base)):
        baseNeg = -base[i]
        if xSigned >= base[i]:
            dcmpOut[i] = 1
            xSigned = xSigned - base[i]
        elif xSigned <= baseNeg:
            dcmpOut[i] = -1
            xSigned = xSigned + base[i]
        else:
            dcmpOut[i] = 0
    return dcmpOut


def residual(x, base, q):
    """What the reference's loop leaves in xSigned (it drops it): centred x - sum_j d_j b_j."""
    xs = x - q if x > (q >> 1) else x
    return xs - sum(d * b for d, b in zip(decomposeBig(x, base, q), base))


def set_int64(ref, v):  # Uint.SetInt64
    return v % ref.q * ref.R % ref.q


# ---- prover.go:77-86 ---------------------------------------------------------------------------------
def infDcmp(ref, w, base):
    """One infinity-norm witness w [rank] -> len(base) digit witnesses [rank] each."""
    rank = len(w)
    wDcmps = [[None] * rank for _ in base]
    for i in range(rank):
        bigCoeff = ref.plain(w[i])  # BigInt
        dcmp = decomposeBig(bigCoeff, base, ref.q)
        for j in range(len(wDcmps)):
            wDcmps[j][i] = set_int64(ref, dcmp[j])
    return wDcmps


# ---- prover.go:88-111 --------------------------------------------------------------------------------
def twoNormPublic(ref, rank, base):
    """prover.go:92-97: (pwBase, pwMask) of one two-norm bound."""
    pwBase, pwMask = [0] * rank, [0] * rank
    for i in range(len(base)):
        pwBase[i] = base[i] % ref.q * ref.R % ref.q  # SetBigInt
        pwMask[i] = set_int64(ref, 1)
    return pwBase, pwMask


def twoDcmp(ref, w, base):
    """One two-norm witness w [rank] -> (the digit witness [rank], sqNm as a plain int).  The
    reference keeps one sqNm across its loop over the bounds; this is its first pass, the sum of
    the witness at hand."""
    rank = len(w)
    sqNm = 0
    for i in range(rank):
        bigCoeff = ref.plain(w[i])
        mul = bigCoeff * bigCoeff
        sqNm = sqNm + mul
    sqNm = sqNm % ref.q
    dcmp = decomposeBig(sqNm, base, ref.q)
    wDcmp = [0] * rank  # the witness starts zeroed (prover.go:65-70)
    for i in range(len(dcmp)):
        wDcmp[i] = set_int64(ref, dcmp[i])
    return wDcmp, sqNm


# ---- prover.go:182-192 -------------------------------------------------------------------------------
def projDcmp(ref, w, base, rank):
    """The projected witness w (its first 128 entries are read) -> the digit witness [rank]."""
    wDcmp = [0] * rank
    for i in range(128):
        bigCoeff = ref.plain(w[i])
        dcmp = decomposeBig(bigCoeff, base, ref.q)
        for j in range(len(base)):
            wDcmp[i * len(base) + j] = set_int64(ref, dcmp[j])
    return wDcmp
