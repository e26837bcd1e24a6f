// Which quad a detection row describes: the rule lp_crops.hip (the crops) and lp_redact.hip (the redaction) share; include inside
// an unnamed namespace of namespace lp.  The specification is yolov6/utils/plate_crop.py::plate_quad: the four predicted corners
// (columns 4..11, label order TL, BL, BR, TR) when they are finite, strictly convex in label orientation and of area >= 1 px^2,
// otherwise the box (columns 0..3) when it is finite and at least 1 px on each side.  fp64 on the row's fp32 values.
__device__ __forceinline__ bool finite4(const double v[4]) {
    return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]);
}

// Quad of one detection row into x[4], y[4] (p0 = TL, p1 = TR, p2 = BR, p3 = BL); returns the status: 1 corners, 2 box, 3 none.
__device__ __forceinline__ int plate_quad(const float* row, double x[4], double y[4]) {
    // corners: TL (c4,c5), TR (c10,c11), BR (c8,c9), BL (c6,c7)
    x[0] = row[4]; y[0] = row[5];
    x[1] = row[10]; y[1] = row[11];
    x[2] = row[8]; y[2] = row[9];
    x[3] = row[6]; y[3] = row[7];
    if (finite4(x) && finite4(y)) {
        // label orientation TL -> BL -> BR -> TR = p0 -> p3 -> p2 -> p1: every cross product of consecutive edges < 0
        const int ord[4] = {0, 3, 2, 1};
        bool convex = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i0 = ord[k], i1 = ord[(k + 1) & 3], i2 = ord[(k + 2) & 3];
            const double ex = x[i1] - x[i0], ey = y[i1] - y[i0];
            const double fx = x[i2] - x[i1], fy = y[i2] - y[i1];
            if (!(ex * fy - ey * fx < 0.0)) convex = false;
        }
        const double area = 0.5 * fabs((x[2] - x[0]) * (y[3] - y[1]) - (x[3] - x[1]) * (y[2] - y[0]));
        if (convex && area >= 1.0) return 1;
    }
    const double x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
    if (isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && x2 - x1 >= 1.0 && y2 - y1 >= 1.0) {
        x[0] = x1; y[0] = y1;
        x[1] = x2; y[1] = y1;
        x[2] = x2; y[2] = y2;
        x[3] = x1; y[3] = y2;
        return 2;
    }
    return 3;
}
