// dropin_tsdffusion_track.cpp -- `class TSDFfusion` estimating its own poses: SetPose for the first frame only, then the
// reference's pose-less call, Integrate(imRGB, imD) (ref: include/TSDFfusion.hpp:49), through the OpenCV-free overloads of
// include/TSDFfusion.hpp.  Input file: int32 n, int32 estimate (0 / 1), int32 with_rgb (0 / 1), float cam2world[16] of the
// first frame, n x { float depth[480*640], uint8 rgb[480*640*3] }.  Output file (argv[2]): per frame int32 LastTrackStatus(),
// float Pose()[16].
#include <cstdio>
#include <vector>

#include "TSDFfusion.hpp"

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	FILE *fp = std::fopen(argv[1], "rb");
	FILE *out = std::fopen(argv[2], "wb");
	if (!fp || !out) return 2;
	int n = 0, estimate = 0, with_rgb = 0;
	float pose[16];
	if (std::fread(&n, 4, 1, fp) != 1 || std::fread(&estimate, 4, 1, fp) != 1 || std::fread(&with_rgb, 4, 1, fp) != 1 ||
	    std::fread(pose, 4, 16, fp) != 16)
		return 2;
	TSDFfusion *tsdf = new TSDFfusion();
	if (tsdf->LastTrackStatus() != -1) return 3;
	tsdf->SetPose(pose);
	tsdf->EstimatePose(estimate != 0);
	std::vector<float> depth(480 * 640);
	std::vector<unsigned char> rgb(480 * 640 * 3, 0);
	for (int k = 0; k < n; ++k) {
		if (std::fread(depth.data(), 4, depth.size(), fp) != depth.size() || std::fread(rgb.data(), 1, rgb.size(), fp) != rgb.size())
			return 2;
		tsdf->Integrate(with_rgb ? rgb.data() : NULL, depth.data(), 480, 640);
		const int status = tsdf->LastTrackStatus();
		if (std::fwrite(&status, 4, 1, out) != 1 || std::fwrite(tsdf->Pose(), 4, 16, out) != 16) return 2;
	}
	std::fclose(fp);
	std::fclose(out);
	delete tsdf;
	return 0;
}
