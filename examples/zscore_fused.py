"""Column z-score standardization with the fused dims-reductions:

    Z .= (X .- mean(X, dims=1)) ./ std(X, dims=1)

examples/zscore.py gets the variance as E[X^2] - mu^2 from a materialised
abs2.(X): 24 bytes moved per element and a form that cancels.  Here
dstd_dims runs the stable two-pass form — the mean row, then ONE fused pass
sum(abs2, X .- mean; dims=1) with the row expanded through its singleton
dim — at 8 bytes per element per pass and with no temporary of X's size.

Run on an MI355X box:  python examples/zscore_fused.py [m] [n]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import distributedarrays_jl_amd as dja
from distributedarrays_jl_amd import expr as E


def zscore(m=8192, n=4096, offset=0.0):
    X = dja.drand((m, n), "f64")
    if offset:
        dja.map2_scalar_("add", X, X, offset)
    mu = dja.dmean_dims(X, 0)                         # (1, n)
    sig = dja.dstd_dims(X, 0, corrected=False)        # (1, n), same owners
    Z = dja.DArray((m, n), "f64")
    E.materialize_(Z, (E.ref(X) - E.ref(mu)) / E.ref(sig))
    return X, mu, sig, Z


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    # a large common offset: E[X^2] - mu^2 would lose 12 digits here
    X, mu, sig, Z = zscore(m, n, offset=1.0e6)
    hX = X.collect().astype(np.longdouble)
    ref_sig = np.std(hX, axis=0, keepdims=True)
    rel = float(np.max(np.abs(sig.collect() - ref_sig) / ref_sig))
    print("zscore_fused %dx%d: max rel err of std vs numpy longdouble = %.3g"
          % (m, n, rel))
    assert rel < 1e-9
    ref = (hX - hX.mean(axis=0, keepdims=True)) / ref_sig
    err = float(np.max(np.abs(Z.collect() - ref)))
    print("max |err| of Z = %.3g" % err)
    assert err < 1e-8
    for d in (X, mu, sig, Z):
        d.close()
    print("ok")


if __name__ == "__main__":
    main()
