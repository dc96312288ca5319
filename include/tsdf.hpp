// tsdf.hpp -- drop-in replacement for the reference's include/tsdf.hpp (class TSDF).
//
// Same class name, same three public methods, same two public data members as
// ref: include/tsdf.hpp:22-43, so the call sites in ref: src/Object.cpp:67-68,76,164 compile and
// behave unchanged:
//     tsdf = new TSDF(mnHeight, mnWidth, mnId, base2world, origin);
//     tsdf->Integrate(depth, cam2world_vec);
//     delete(tsdf);          // writes tsdf<id>.ply and tsdf<id>.bin in the working directory
// Unlike the reference header this one needs neither cuda_runtime.h nor OpenCV
// (ref: include/tsdf.hpp:8,15-16): it is plain C++11 over the C ABI in tsdf_hip.h, and the
// arithmetic runs in hand-written HIP kernels on an MI355X (libtsdf_hip.so).
//
// Additions the reference lacks (all optional; defaults reproduce the reference):
//     TSDF(const tsdf_config&)   run-time grid size / voxel size / intrinsics / z-slab / device
//     TSDF(const tsdf_config&, devices)   the same grid cut into z-slabs over several GPUs of the node, in this
//                                process (tsdf_group_*): Integrate fans the frame out, the destructor gathers
//     IntegrateRange(), IntegrateScan()   Integrate for the reference's second sensor (mSensor == 1): an image of lidar
//                                ranges, or the Velodyne scan itself, made into z-depth on the device
//     TrackScan()                estimate the pose IntegrateScan needs from the scan and the volume themselves, point to signed
//                                distance (csrc/tsdf_scan_track.hip.h): the lidar path's own tracker
//     SetScanFill(), ClearScanFill()   fill the gaps between lidar beams in front of IntegrateRange / IntegrateScan
//                                (csrc/tsdf_scan_fill.hip.h); off by default
//     SetScanGround(), ClearScanGround()   mark the ground of a scan and keep it out of (or alone in) IntegrateScan
//                                (csrc/tsdf_scan_ground.hip.h); off by default
//     Download(), Sync()         read results back without destroying the object
//     SetSaveOnDestroy(false)    skip the two files the destructor writes
//     TSDF::ThrowOnError(true)   throw std::runtime_error instead of print + exit(1)
#ifndef TSDF_HIP_DROPIN_TSDF_HPP
#define TSDF_HIP_DROPIN_TSDF_HPP

#include <string>
#include <vector>

#include "tsdf_hip.h"

class TSDF
{
	public:

	/** Object TSDF constructor (ref: include/tsdf.hpp:30, src/tsdf.cu:62-96)
	@param h depth image height
	@param w depth image width
	@param id object id, names the files written at destruction
	@param base2world_vec 16 floats, row-major pose of the base camera (first keyframe's Twc)
	@param origin 3 floats, grid origin in the base camera frame
	Grid: the reference's compile-time 200^3 voxels of 4 mm, truncation 20 mm, TUM fr3 intrinsics.
	*/
	TSDF(int h, int w, int id, std::vector<float> base2world_vec, std::vector<float> origin);

	/** Run-time configured volume (not in the reference). */
	explicit TSDF(const tsdf_config &cfg);

	/** The grid of cfg cut into devices.size() contiguous z-slabs, slab i on HIP device devices[i] (not in the
	reference, which is single-GPU).  Same Integrate / Download / destructor behaviour; results and files are
	bit-identical to the single-device object. */
	TSDF(const tsdf_config &cfg, const std::vector<int> &devices);

	/** Downloads the grid, writes tsdf<id>.ply and tsdf<id>.bin (ref: src/tsdf.cu:98-133). */
	~TSDF();

	/** Integrate one depth image (ref: include/tsdf.hpp:37, src/tsdf.cu:135-168)
	@param depth_im pointer to h*w floats, metres, row-major; borrowed for the call only
	@param cam2world_vec 16 floats, row-major camera pose
	*/
	void Integrate(float *depth_im, std::vector<float> cam2world_vec);

	/** Integrate one image of lidar RANGES, distances along the ray (not in the reference, whose lidar call site hands its
	range image to Integrate as it is: ref: examples/label_instance_lidar.cpp:76-77,126, src/Object.cpp:160-164 and the FIXME
	at :41).  Each range is divided by its ray's length under the object's intrinsics (ref: src/Object.cpp:613-620), on the
	device, and the z-depth image is integrated as Integrate would.
	@param range_im pointer to h*w floats, metres along the ray, 0 = no return; borrowed for the call only
	*/
	void IntegrateRange(float *range_im, std::vector<float> cam2world_vec);

	/** Integrate one Velodyne scan (ref: src/Utility.cpp:374-419 makes the range image of it on the CPU).
	@param xyzi n points of 4 floats (x, y, z, intensity) in the scanner's frame, the KITTI .bin layout; borrowed for the call
	@param n number of points
	@param velo2img 12 floats, row-major 3x4: scanner frame to pixels times depth (tsdf_scan_projection composes it)
	*/
	void IntegrateScan(const float *xyzi, size_t n, const float velo2img[12], std::vector<float> cam2world_vec);

	/** Refine the camera pose of one Velodyne scan against the fused volume (not in the reference, which takes every pose of
	its lidar call site from a stereo SLAM run: ref: examples/label_instance_lidar.cpp:36-40): tsdf_scan_track with
	tsdf_scan_track_params_default, started from velo2world = cam2world_vec * velo2cam.  With SetScanGround on, the scan's
	ground is marked first and left out of the tracking (drop_flag 1, whatever select says).  The volume is only read.
	@param xyzi, n the scan as IntegrateScan takes it
	@param velo2cam 16 floats, row-major 4x4: scanner frame to camera frame (tsdf_scan_pose composes it)
	@param cam2world_vec in: the guess; out: the refined pose, velo2world * inverse(velo2cam) in tsdf_multiply_matrix's order
	@return false when the track is lost (or velo2cam is singular): cam2world_vec is then left as it was
	A multi-device object is refused: tracking needs the whole grid on one device.
	*/
	bool TrackScan(const float *xyzi, size_t n, const float velo2cam[16], std::vector<float> &cam2world_vec);

	/** From here on IntegrateRange and IntegrateScan fill the gaps between beams in their z-depth image before it is
	integrated (not in the reference, whose lidar call site fuses the sparse image): inverse depth is interpolated between
	the nearest sources at most max_span_u pixels apart along rows, then at most max_span_v apart along columns, never
	across a relative depth difference above jump_rel (tsdf_scan_fill_params in tsdf_hip.h; its defaults are 5, 8, 0.05f).
	Parameters outside their range make the next IntegrateRange / IntegrateScan fail.  Integrate is not touched.
	*/
	void SetScanFill(int max_span_u, int max_span_v, float jump_rel);
	/// back to the default: IntegrateRange and IntegrateScan integrate the sparse image as it is
	void ClearScanFill() { fill_on_ = false; }

	/** From here on IntegrateScan marks the ground of each scan on the device first (not in the reference, whose lidar call
	site has projectPointCloud and groundRemoval dormant: ref: examples/label_instance_lidar.cpp:85-91, src/Utility.cpp:452-553)
	and integrates only the points that select keeps: TSDF_SCAN_DROP_GROUND everything but the ground returns,
	TSDF_SCAN_ONLY_GROUND nothing else (tsdf_scan_ground_params in tsdf_hip.h; tsdf_scan_ground_params_default gives the
	reference's literals, which do not fit an HDL-64E: see there).  With SetScanFill the fill runs behind the selection.
	Parameters outside their range make the next IntegrateScan fail.  IntegrateRange takes an image, which has no points
	to mark, and is unaffected; so is Integrate.
	*/
	void SetScanGround(const tsdf_scan_ground_params &params, int select = TSDF_SCAN_DROP_GROUND);
	/// back to the default: IntegrateScan integrates every point
	void ClearScanGround() { ground_on_ = false; }

	/// pointer to a TSDF voxel grid (host mirror; refreshed by Download() and by the destructor)
	float * voxel_grid_TSDF;

	/// pointer to a TSDF voxel grid weights (host mirror)
	float * voxel_grid_weight;

	// ---- additions -------------------------------------------------------------------------
	void Download();                        ///< refresh the two host mirrors now
	void Sync();                            ///< wait for queued integrations
	void SetSaveOnDestroy(bool on) { save_on_destroy_ = on; }
	tsdf_volume *handle() const { return vol_; }   ///< NULL for a multi-device object
	tsdf_group *group() const { return grp_; }     ///< NULL for a single-device object
	const tsdf_config &config() const { return cfg_; }
	static void ThrowOnError(bool on);      ///< default false: print to stderr and exit(EXIT_FAILURE)

	private:

	TSDF(const TSDF &);             // one object owns one device volume (the reference never copies it)
	TSDF &operator=(const TSDF &);
	void init();
	int download_mirrors();
	void fail(const char *what, int line) const;
	void fail_in_destructor(const char *what, int line) const;   // never throws (ThrowOnError: prints and goes on)
	long long voxels() const;
	tsdf_config cfg_;
	tsdf_volume *vol_;
	tsdf_group *grp_;
	std::vector<int> devices_;
	bool save_on_destroy_;
	tsdf_scanner *scan_;               // a multi-device object's: scans become z-depth on devices_[0], then fan out
	std::vector<float> scan_depth_;
	float *scan_image();               // scan_ and scan_depth_ at their first use
	bool fill_on_;                     // SetScanFill: the lidar calls go through the library's filled forms
	tsdf_scan_fill_params fill_;
	bool ground_on_;                   // SetScanGround: IntegrateScan goes through the library's selecting forms
	tsdf_scan_ground_params ground_;
	int ground_select_;
	std::vector<unsigned char> scan_flags_;   // TrackScan with SetScanGround: the scan's flags
};
#endif // TSDF_HIP_DROPIN_TSDF_HPP
