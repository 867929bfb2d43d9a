// csrc/sos_polar.h -- SOS_POLAR (reference src/SOS_TRPHI.F:1843) and the output thresholds of SOS_TRPHI (:1212-1218), shared by
// the azimuth recomposition (trphi.hip) and the channel sums of a spectrum (channels.hip).  Include it behind
// `#pragma clang fp contract(off)`: both callers are held to the bits of these statements.
#pragma once

#define THRESHOLD_Q_U_NULL 1.e-15      // SOS.h:418
#define VALEUR_INDEF (-999.)

// SOS_TRPHI.F:1212-1218: what the reference zeroes before it writes XIT, XQT, XUT
__device__ __forceinline__ void sos_trphi_thresholds(double &xit, double &xqt, double &xut)
{
    if (xit <= 1.e-99) xit = 0.0;
    if (fabs(xqt) < THRESHOLD_Q_U_NULL) xqt = 0.0;
    if (fabs(xut) < THRESHOLD_Q_U_NULL) xut = 0.0;
}

// SOS_POLAR :1865-1903: polarisation angle (deg), polarisation rate (%) and polarised radiance of (XIT, XQT, XUT)
__device__ __forceinline__ void sos_polar(const double xit, const double xqt, const double xut, double &xan, double &tpol,
                                          double &lpol)
{
    const double pi = acos(-1.0);
    if (xqt != 0.) {
        const double xt = xut / xqt;
        if (xqt > 0.) xan = 90. * atan(xt) / pi;
        else if (xut > 0.) xan = 90. + 90. * atan(xt) / pi;
        else xan = -90. + 90. * atan(xt) / pi;
    } else {
        if (xut > 0.) xan = 45.;
        else if (xut < 0) xan = -45.;
        else xan = VALEUR_INDEF;
    }
    lpol = sqrt(xqt * xqt + xut * xut);
    tpol = (xit != 0.0) ? 100. * lpol / xit : VALEUR_INDEF;
}
