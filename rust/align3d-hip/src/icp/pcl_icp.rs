//! `Icp` (replaces src/icp/pcl_icp.rs:31-107): kd-tree point-to-plane ICP; the tree is built on the device by `new`.
use crate::{device, sys};
use align3d::{icp::IcpParams, pointcloud::PointCloud, transform::Transform};

pub struct Icp<'target> {
    pub params: IcpParams,
    /// Kept for API compatibility: the reference's `align` ignores it too (pcl_icp.rs:59).
    pub initial_transform: Transform,
    target: &'target PointCloud,
    handle: *mut sys::a3d_pcl_icp,
}

fn view_of(pcl: &PointCloud) -> sys::a3d_point_cloud_view {
    sys::a3d_point_cloud_view {
        points: pcl.points.as_ptr() as *const f32, // Array1<Vector3<f32>>: 12-byte stride
        normals: pcl.normals.as_ref().map_or(std::ptr::null(), |n| n.as_ptr() as *const f32),
        len: pcl.len() as u64,
    }
}

impl<'target> Icp<'target> {
    /// src/icp/pcl_icp.rs:31-38: builds the kd-tree over `target.points` (panics on a NaN coordinate like
    /// `partial_cmp().unwrap()`, kdtree.rs:43).
    pub fn new(params: IcpParams, target: &'target PointCloud) -> Self {
        let ctx = device::Context::current();
        let (c_params, view) = (device::params_of(&params), view_of(target));
        let mut handle = std::ptr::null_mut();
        device::check(unsafe { sys::a3d_pcl_icp_new(ctx, &c_params, &view, &mut handle) }, "Icp::new");
        Self { params, initial_transform: Transform::eye(), target, handle }
    }

    /// src/icp/pcl_icp.rs:49-107.  Panics like the reference when either cloud has no normals (`expect`, :50-58)
    /// or `solve()` returns `None` (:96).
    pub fn align(&self, source: &PointCloud) -> Transform {
        let _ = self.target;
        let view = view_of(source);
        let mut pose = sys::a3d_pose::default();
        device::check(unsafe { sys::a3d_pcl_icp_align(self.handle, &view, &mut pose) }, "Icp::align");
        device::transform_of(&pose)
    }
}

/// P independent `Icp::new(params, target_p).align(source_p)` over clouds that are resident in device memory, as one
/// launch sequence (a3d_pcl_icp_batch_*).  No counterpart in the reference.  The views hold DEVICE pointers; the
/// caller keeps the clouds alive while the batch reads them (targets: during `new`; sources: during `align`).
pub struct IcpBatch {
    n_pairs: usize,
    handle: *mut sys::a3d_pcl_icp_batch,
}

impl IcpBatch {
    /// Builds the P kd-trees behind one host wait.  Panics where `Icp::new` / `align` would (NaN coordinate,
    /// kdtree.rs:43; target without normals, pcl_icp.rs:50-53).
    pub fn new(params: &IcpParams, device_targets: &[sys::a3d_point_cloud_view]) -> Self {
        let ctx = device::Context::current();
        let c_params = device::params_of(params);
        let mut handle = std::ptr::null_mut();
        device::check(
            unsafe {
                sys::a3d_pcl_icp_batch_new_device(ctx, &c_params, device_targets.len() as u64, device_targets.as_ptr(),
                                                  &mut handle)
            },
            "IcpBatch::new",
        );
        Self { n_pairs: device_targets.len(), handle }
    }

    /// One transform per pair; `None` where the reference's `solve().unwrap()` (pcl_icp.rs:96) would panic: a failed
    /// pair does not disturb the others.
    pub fn align(&self, device_sources: &[sys::a3d_point_cloud_view]) -> Vec<Option<Transform>> {
        assert_eq!(device_sources.len(), self.n_pairs, "one source per pair of the batch");
        let mut poses = vec![sys::a3d_pose::default(); self.n_pairs];
        let mut status = vec![0i32; self.n_pairs];
        device::check(
            unsafe {
                sys::a3d_pcl_icp_batch_align_device(self.handle, device_sources.as_ptr(), poses.as_mut_ptr(),
                                                    status.as_mut_ptr())
            },
            "IcpBatch::align",
        );
        poses.iter().zip(&status).map(|(p, s)| (*s == sys::A3D_OK).then(|| device::transform_of(p))).collect()
    }
}

impl Drop for IcpBatch {
    fn drop(&mut self) {
        unsafe { sys::a3d_pcl_icp_batch_free(self.handle) };
    }
}

impl Drop for Icp<'_> {
    fn drop(&mut self) {
        unsafe { sys::a3d_pcl_icp_free(self.handle) };
    }
}
