# CMTCoop vehicle + infrastructure LiDAR only, TUMTraf shapes.
# Head block of the reference's CMTCoop_TUMTraf/lidar/coop/cmt_lidar_voxel0075_cbgs_a9coop_pretrained.py:167-297.
point_cloud_range = [-72.0, -72.0, -8, 72.0, 72.0, 0]
voxel_size = [0.1, 0.1, 0.2]
tumtraf_classes = ['CAR', 'TRAILER', 'TRUCK', 'VAN', 'PEDESTRIAN', 'BUS', 'BICYCLE']
grid_size = [1440, 1440, 40]
pts_voxel_layer = dict(num_point_features=5, max_num_points=10, voxel_size=voxel_size,
                       max_voxels=(120000, 160000), point_cloud_range=point_cloud_range)
head_type = 'CmtLidarHeadCoop'
transformer_type = 'CmtLidarTransformer'
final_kernel = 3
post_center_range = [-80, -80, -10.0, 80, 80, 10.0]
# The point steps of the reference's test pipeline (CMTCoop_TUMTraf/lidar/coop/cmt_lidar_voxel0075_cbgs_a9coop_pretrained.py:
# 94-120), read by native_pts.points_plan_from_config.
data = dict(test=dict(pipeline=[
    dict(type='LoadPointsFromFileCoop', coord_type='LIDAR', load_dim=5, use_dim=[0, 1, 2, 3, 4]),
    dict(type='LoadPointsFromMultiSweepsCoop', sweeps_num=10, use_dim=[0, 1, 2, 3, 4]),
    dict(type='VehiclePointsToInfraCoords'),
    dict(type='MultiScaleFlipAug3D', pts_scale_ratio=1, flip=False, transforms=[
        dict(type='GlobalRotScaleTransCoop', rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
        dict(type='PointsRangeFilterCoop', point_cloud_range=point_cloud_range),
    ]),
]))
