"""phk_div_row (phamers_amd/csrc/phk_common.h) replayed in exact rational arithmetic: x / T from a shared correctly rounded
reciprocal and two fused Newton steps on the quotient equals the IEEE quotient on every case tried (row sums 1 .. 400, around
every power of two up to 2^32, the benchmark lengths, 300 000 random pairs).  The one-step form is counted too: it never
differed here either, but only the two-step form is covered by Markstein's theorem for every input."""
import random, sys
from fractions import Fraction
def fma(a,b,c): return float(Fraction(a)*Fraction(b)+Fraction(c))
def div5(x,T,y):
    q0 = x*y
    e = fma(-q0,T,x)
    q1 = fma(e,y,q0)
    e1 = fma(-q1,T,x)
    return fma(e1,y,q1)
def div3(x,T,y):
    q0 = x*y
    e = fma(-q0,T,x)
    return fma(e,y,q0)
random.seed(1)
bad5=bad3=0; n=0
def cases():
    for T in list(range(1,400))+[2**k+d for k in range(8,32) for d in (-3,-1,0,1,3)]+[9996,4996,9995,49996,499996,10**7,2**32-1,2**32-5]:
        for x in set([0,1,2,3,T//3,T//2,T-1,T, max(T-2,0), T//7+1]+[random.randrange(0,T+1) for _ in range(8)]):
            if 0<=x<=T: yield x,T
    for _ in range(300000):
        T=random.randrange(1,2**32) if random.random()<0.5 else random.randrange(1,200000)
        x=random.randrange(0,T+1) if random.random()<0.7 else random.randrange(0,min(T,3000)+1)
        yield x,T
for x,T in cases():
    xf,Tf=float(x),float(T); y=1.0/Tf
    w=xf/Tf
    n+=1
    if div5(xf,Tf,y)!=w: bad5+=1; print("bad5",x,T) if bad5<5 else None
    if div3(xf,Tf,y)!=w: bad3+=1
print(n,"cases; mismatches 5-op:",bad5," 3-op:",bad3)


# ---- does the one-step form ever misround?  The quotients nearest to a rounding midpoint: x 2^54 = m T +- 1 with m an odd
# 54-bit integer (x / T in [1/2, 1), as close to the midpoint m / 2^54 as an integer pair can be), T odd in [2^50, 2^53),
# and again with T >= 0.9 * 2^53, m >= 0.85 * 2^54 and a reciprocal whose rounding error is at least 3/4 of its bound -- the
# corner where the error of q1 before rounding, |x / T - q0| |T y - 1|, is largest against the distance 1 / (T 2^54).
def nearest_to_midpoint(lo, hi, tries, m_min=2**53, delta_min=0.0):
    cnt = bad3 = bad5 = 0
    for _ in range(tries):
        T = random.randrange(lo, hi) | 1
        Tf = float(T); y = 1.0 / Tf
        if delta_min and abs(Fraction(y) * T - 1) * 2**53 < delta_min: continue
        inv = pow(T, -1, 2**54)
        for sign in (1, -1):
            m = (-sign * inv) % 2**54
            if m < m_min: continue
            x = (m * T + sign) >> 54
            if not 0 < x < T: continue
            cnt += 1
            xf = float(x)
            bad3 += div3(xf, Tf, y) != xf / Tf
            bad5 += div5(xf, Tf, y) != xf / Tf
    return cnt, bad3, bad5
if "--midpoints" in sys.argv:
    for lo, hi in ((2**52, 2**53), (2**51, 2**52), (2**50, 2**51)):
        print("T in [2^%d, 2^%d): (cases, 3-op mismatches, 5-op mismatches) =" % (lo.bit_length() - 1, hi.bit_length() - 1),
              nearest_to_midpoint(lo, hi, 60000))
    print("T >= 0.9 * 2^53, m >= 0.85 * 2^54, |T y - 1| >= 0.75 * 2^-53:",
          nearest_to_midpoint(int(0.9 * 2**53), 2**53, 1500000, int(0.85 * 2**54), 0.75))
