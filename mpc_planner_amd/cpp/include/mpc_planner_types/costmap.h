/*
 * mpc_planner_types/costmap.h -- the little of costmap_2d::Costmap2D that DecompConstraints::getOccupiedGridCells reads
 * (decomp_constraints.cpp:122-148): the size in cells, a cell's cost, the world position of a cell's centre and FREE_SPACE.  A full tree
 * passes its own costmap_2d::Costmap2D instead: FreeSpace::occupiedCells (mpc_planner_modules/free_space.h) takes any class with these
 * members.  Storage is costmap_2d's: index my * size_x + mx.
 */
#ifndef MPC_COSTMAP_HIP_H
#define MPC_COSTMAP_HIP_H

#include <cstdint>
#include <vector>

#include <mpc_planner_types/prep_arithmetic.h>

namespace costmap_2d
{
    static const unsigned char NO_INFORMATION = 255;
    static const unsigned char LETHAL_OBSTACLE = 254;
    static const unsigned char INSCRIBED_INFLATED_OBSTACLE = 253;
    static const unsigned char FREE_SPACE = 0;

    class Costmap2D
    {
    public:
        Costmap2D() = default;
        Costmap2D(unsigned int cells_size_x, unsigned int cells_size_y, double resolution, double origin_x, double origin_y, unsigned char default_value = 0)
            : size_x_(cells_size_x), size_y_(cells_size_y), resolution_(resolution), origin_x_(origin_x), origin_y_(origin_y),
              costmap_((size_t)cells_size_x * cells_size_y, default_value) {}

        unsigned int getSizeInCellsX() const { return size_x_; }
        unsigned int getSizeInCellsY() const { return size_y_; }
        double getResolution() const { return resolution_; }
        double getOriginX() const { return origin_x_; }
        double getOriginY() const { return origin_y_; }
        unsigned char getCost(unsigned int mx, unsigned int my) const { return costmap_[(size_t)my * size_x_ + mx]; }
        void setCost(unsigned int mx, unsigned int my, unsigned char cost) { costmap_[(size_t)my * size_x_ + mx] = cost; }
        /* the centre of cell (mx, my): origin + (m + 0.5) resolution */
        void mapToWorld(unsigned int mx, unsigned int my, double &wx, double &wy) const
        {
            wx = tmpc_arith::cell_centre(origin_x_, (int)mx, resolution_);
            wy = tmpc_arith::cell_centre(origin_y_, (int)my, resolution_);
        }
        const unsigned char *getCharMap() const { return costmap_.data(); }
        unsigned char *getCharMap() { return costmap_.data(); }

    private:
        unsigned int size_x_{0}, size_y_{0};
        double resolution_{0.}, origin_x_{0.}, origin_y_{0.};
        std::vector<unsigned char> costmap_;
    };
}
#endif
